"""Where trained heads go when the fp16 plan's guard repeats a forward in its fp32 sibling: ``ops.Net.set_param_device`` against a
stub of the C library (no GPU; the handles are integers and the tensors live on the CPU, as in tests/test_f16_guard_host.py)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from happypose_amd import ops
from test_f16_guard_host import StubLib


class Stub(StubLib):
    def __init__(self):
        super().__init__()
        self.sets = []  # (handle, name, data pointer, numel) in call order

    def hp_net_set_param_device(self, h, name, p, numel, stream):
        self.sets.append((h.value, name.decode(), p.value, numel))
        return 0


@pytest.fixture
def stub(monkeypatch):
    lib = Stub()
    monkeypatch.setattr(ops, "lib", lambda: lib)
    monkeypatch.setattr(ops, "stream_ptr", lambda dev: C.c_void_p(0))
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    return lib


def _net(precision):
    w = {"conv.weight": np.ones((4, 9, 3, 3), np.float32), "pose_fc.weight": np.ones((9, 512), np.float32),
         "pose_fc.bias": np.ones(9, np.float32)}
    return ops.Net("resnet34", 9, w, max_batch=8, device="cpu", h=8, w=8, precision=precision)


def test_heads_set_before_the_sibling_exists_reach_it_when_it_is_built(stub):
    net = _net("f16")
    W, b = torch.zeros(9, 512), torch.zeros(9)
    net.set_param_device("pose_fc.weight", W)
    net.set_param_device("pose_fc.bias", b)
    assert stub.sets == [(1, "pose_fc.weight", W.data_ptr(), 9 * 512), (1, "pose_fc.bias", b.data_ptr(), 9)] and stub.created == [1]
    W2 = torch.ones(9, 512)
    net.set_param_device("pose_fc.weight", W2)  # a later step: the newest tensor is the one a sibling must get
    del stub.sets[:]
    stub.fire.add(1)
    net.status()  # the guard fires: the sibling is built from the STALE host parameters, then given the trained heads
    assert stub.created == [1, 2]
    assert sorted(stub.sets) == sorted([(2, "pose_fc.weight", W2.data_ptr(), 9 * 512), (2, "pose_fc.bias", b.data_ptr(), 9)])


def test_heads_set_after_the_sibling_exists_go_to_both_plans(stub):
    net = _net("f16")
    net.force_exact(True)
    assert stub.created == [1, 2] and stub.sets == []
    W = torch.zeros(9, 512)
    net.set_param_device("pose_fc.weight", W)  # while on the sibling ...
    net.force_exact(False)
    net.set_param_device("pose_fc.weight", W)  # ... and back on the fp16 plan
    assert stub.sets == [(1, "pose_fc.weight", W.data_ptr(), 9 * 512), (2, "pose_fc.weight", W.data_ptr(), 9 * 512)] * 2


def test_an_fp32_network_keeps_nothing(stub):
    net = _net("f32")
    W = torch.zeros(9, 512)
    net.set_param_device("pose_fc.weight", W)
    assert stub.sets == [(1, "pose_fc.weight", W.data_ptr(), 9 * 512)] and net._device_params is None
    with pytest.raises(AssertionError):
        net.set_param_device("pose_fc.weight", W.double())


def test_head_param_shapes_follow_the_architecture(stub):
    assert _net("f32").head_param_shapes() == {"pose_fc.weight": (9, 512), "pose_fc.bias": (9,)}
    w = {"pose_fc.weight": np.ones((9, 512), np.float32), "views_logits_head.weight": np.ones((4, 512), np.float32)}
    net = ops.Net("vanilla_resnet34", 9, w, max_batch=8, device="cpu", h=8, w=8)
    assert list(net.head_param_shapes()) == ["backbone.fc.weight", "backbone.fc.bias", "pose_fc.weight", "pose_fc.bias",
                                             "views_logits_head.weight", "views_logits_head.bias"]
