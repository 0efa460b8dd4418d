"""The conv kernel choice, pinned: what every op of the ResNet plans and of EfficientNet-b3 launches, op by op,
against ``tests/golden/net_paths.json`` -- the path part of a ``tools/net_paths.py`` dump, recorded before the choice moved
into ``choose_conv``.  The golden is the record: a network that disagrees with it launches something else than it did."""

import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

GRID = [(a, c, "f32", ("auto", "winograd", "igemm")) for a, c in (("vanilla_resnet34", 9), ("resnet34", 6), ("resnet18", 6), ("efficientnet-b3", 6))] + \
       [(a, c, "f16", ("auto",)) for a, c in (("vanilla_resnet34", 9), ("resnet34", 6), ("resnet18", 6))]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "net_paths.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("arch,cin,precision,algos", GRID, ids=[f"{a}-{c}-{p}" for a, c, p, _ in GRID])
def test_paths_match_the_golden(golden, arch, cin, precision, algos):
    import net_paths

    assert torch.cuda.is_available(), "run on the MI355X box"
    got = net_paths.run_net(arch, cin, precision, torch.device("cuda:0"), algos=algos, exact=(False,))
    assert len(got) == len(algos)
    for key, rec in got.items():
        key = "plain/" + key
        assert rec["status"] == 0, key
        want = net_paths.golden_ops(golden, key)
        diff = [(i, w, g) for i, (w, g) in enumerate(zip(want, rec["ops"])) if w != g]
        assert len(want) == len(rec["ops"]) and not diff, (key, diff[:5])
        # the accounting of the same launches: launch count and the two FLOP sums, bit for bit
        assert rec["profile"] == golden["records"][key]["profile"], key
