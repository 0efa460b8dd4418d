"""Switch-over logic of ``ops.Net(precision="f16")`` (the fp32 sibling the numerical guard falls back to) against a stub of the
C library: no GPU, no GPU runtime -- the network "handles" are integers and the tensors live on the CPU."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from happypose_amd import ops


class StubLib:
    """What ``ops.Net`` calls, recorded.  ``fire`` holds the handles whose next ``hp_net_status`` reports NONFINITE."""

    def __init__(self):
        self.created, self.precision, self.fire, self.exact, self.calls = [], {}, set(), {}, []

    def hp_net_create(self, arch, n_inputs, h, w):
        self.created.append(len(self.created) + 1)
        return self.created[-1]

    def hp_net_set_param(self, h, name, p, n):
        return 0

    def hp_net_set_precision(self, h, prec):
        self.precision[h.value] = prec
        return 0

    def hp_net_finalize(self, h, max_batch):
        return 0

    def hp_net_input_channels_padded(self, h):
        return 12

    def hp_net_input_channels_f16(self, h):
        return 16 if self.precision[h.value] == 1 else -1

    def hp_net_flops_per_sample(self, h):
        return 1.0

    def hp_net_destroy(self, h):
        return 0

    def hp_net_force_exact(self, h, on):
        self.exact[h.value] = bool(on)
        return 0

    def hp_net_set_tail_split(self, h, on):
        self.calls.append(("tail_split", h.value, on))
        return 0

    def hp_net_set_profiling(self, h, on):
        self.calls.append(("profiling", h.value, on))
        return 0

    def hp_net_status(self, h, stream, flags):
        f16 = self.precision[h.value] == 1
        v = 0
        if h.value in self.fire:
            self.fire.discard(h.value)
            v |= ops.STATUS_NONFINITE
            if not f16:
                self.exact[h.value] = True
        if self.exact.get(h.value) and not f16:  # as the library: an fp16 network never reports EXACT_ONLY
            v |= ops.STATUS_EXACT_ONLY
        flags._obj.value = v
        return 0

    def hp_last_error(self):
        return b""


@pytest.fixture
def stub(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(ops, "lib", lambda: lib)
    monkeypatch.setattr(ops, "stream_ptr", lambda dev: C.c_void_p(0))
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    return lib


def _net(precision="f16"):
    w = {"conv.weight": np.ones((4, 9, 3, 3), np.float32), "pose_fc.weight": np.ones((9, 512), np.float32)}
    return ops.Net("vanilla_resnet34", 9, w, max_batch=8, device="cpu", h=8, w=8, precision=precision)


def test_sibling_is_built_once_and_status_follows_the_contract(stub):
    net = _net()
    assert stub.created == [1] and net._sibling is None and net._host_params is not None
    e0 = ops.graph_epoch()
    assert net.status() == 0 and net.status() == 0
    assert ops.graph_epoch() == e0 and stub.created == [1], "a clean fp16 network builds nothing and drops no graph"
    assert net.new_input(2).dtype == torch.float16 and net.input_spec() == (torch.float16, 16)

    stub.fire.add(1)
    assert net.status() == ops.STATUS_NONFINITE | ops.STATUS_EXACT_ONLY  # the firing call
    assert stub.created == [1, 2] and stub.precision[2] == 0 and stub.exact[2] is True  # an fp32 sibling, forced exact
    assert (net._sibling.arch, net._sibling.n_inputs, net._sibling.h, net._sibling.w, net._sibling.max_batch) == \
        (net.arch, net.n_inputs, net.h, net.w, net.max_batch)
    assert ops.graph_epoch() == e0 + 1
    assert net.status() == ops.STATUS_EXACT_ONLY and net.status() == ops.STATUS_EXACT_ONLY  # sticky, nothing flagged
    assert ops.graph_epoch() == e0 + 1, "the sticky bit alone drops no graph"
    x = net.new_input(2)
    assert x.dtype == torch.float32 and x.shape == (2, 8, 8, 12) and net.input_spec() == (torch.float32, 12)

    net.force_exact(True)  # what PoseEstimator._guarded does after the flag: already there
    assert ops.graph_epoch() == e0 + 1 and stub.created == [1, 2]
    net.force_exact(False)
    assert ops.graph_epoch() == e0 + 2 and net.status() == 0 and net.new_input(1).dtype == torch.float16
    net.force_exact(True)  # the sibling is kept: built once
    assert ops.graph_epoch() == e0 + 3 and stub.created == [1, 2] and net.status() == ops.STATUS_EXACT_ONLY


def test_force_exact_builds_the_sibling_and_settings_reach_it(stub):
    net = _net()
    net.set_tail_split(False)
    net.force_exact(True)  # another lane's guard fired
    assert stub.created == [1, 2]
    assert ("tail_split", 2, 0) in stub.calls, "the sibling starts with the lane's tail-split state"
    net.set_tail_split(True)
    assert ("tail_split", 2, 1) in stub.calls and ("tail_split", 1, 1) in stub.calls and net.tail_split
    stub.fire.add(2)  # the sibling's own (split-fp16) guard is still reported through the fp16 front
    assert net.status() == ops.STATUS_NONFINITE | ops.STATUS_EXACT_ONLY


def test_fp32_network_is_unchanged(stub):
    net = _net("f32")
    assert net._host_params is None
    e0 = ops.graph_epoch()
    stub.fire.add(1)
    assert net.status() == ops.STATUS_NONFINITE | ops.STATUS_EXACT_ONLY and stub.created == [1]
    assert ops.graph_epoch() == e0 + 1 and net.status() == ops.STATUS_EXACT_ONLY and ops.graph_epoch() == e0 + 1


def test_predictor_input_buffer_follows_the_backbone(stub):
    from happypose_amd.pose_predictor import PosePredictor

    net = _net()
    pred = object.__new__(PosePredictor)
    pred.backbone, pred._x = net, None
    a = pred._input_buffer(4)
    assert a.dtype == torch.float16 and pred._input_buffer(3).data_ptr() == a.data_ptr()  # reused
    stub.fire.add(1)
    net.status()
    b = pred._input_buffer(2)
    assert b.dtype == torch.float32 and b.shape == (2, 8, 8, 12) and pred._x.shape[0] == 4  # re-made, no smaller than before
    net.force_exact(False)
    assert pred._input_buffer(4).dtype == torch.float16
