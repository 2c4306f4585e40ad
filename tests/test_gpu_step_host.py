"""The buffer cache of the one-call steps (mal_amd.step.byte_workspace / _scale_buffers) and ``workspace_slot``.

A cached buffer belongs to one (kind, device, stream, workspace slot, shape ...): the same request finds it again, any other
gets its own, and it is reallocated only when it is too small.  Two steps in flight on one stream keep their maps apart
under two slots and overwrite each other's without them -- which ``ops.check_workspace`` refuses."""
import pytest
import torch

from mal_amd import _lib as L
from mal_amd.synthetic import make_batch, to_dicts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W = 1, 16, 24


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def test_the_same_request_finds_its_buffer_and_any_other_gets_its_own():
    from mal_amd import step
    dev = torch.device(DEV)
    need = 4096
    requests = {
        "step": lambda: step._workspace(dev, B, H, W),
        "step, other shape": lambda: step._workspace(dev, B, H, W + 8),
        "multiscale": lambda: step.byte_workspace("multiscale", dev, need, B, H, W, 1),
        "multiscale, other sclm": lambda: step.byte_workspace("multiscale", dev, need, B, H, W, 2),
        "dualrefine, scale 0": lambda: step.byte_workspace("dualrefine", dev, need, B, H, W, 2, 0),
        "dualrefine, scale 2": lambda: step.byte_workspace("dualrefine", dev, need, B, H, W, 2, 2),
        "scale hint, teacher": lambda: step._scale_buffers(dev, B, H, W, False, 1)[0],
        "scale hint, student": lambda: step._scale_buffers(dev, B, H, W, True, 1)[0],
        "scale hint, scale 2": lambda: step._scale_buffers(dev, B, H, W, False, 2)[0],
    }
    side = torch.cuda.Stream(device=dev)
    seen = {}
    for name, get in requests.items():
        seen[name] = get()
        assert get() is seen[name], name
        with step.workspace_slot(1):
            seen[name + " / slot 1"] = get()
            assert get() is seen[name + " / slot 1"], name
        with torch.cuda.stream(side):
            seen[name + " / second stream"] = get()
        assert get() is seen[name], name  # the slot and the stream are back
    ptrs = {name: t.data_ptr() for name, t in seen.items()}
    assert len(set(ptrs.values())) == len(ptrs) == 3 * len(requests), ptrs
    pair, pre0, pre1 = step._scale_buffers(dev, B, H, W, False, 1)
    assert pair.shape == (B, 2, 3, H, W) and pre0.shape == pre1.shape == (B, 3, H, W)
    assert step._workspace(dev, B, H, W).numel() >= L.load().mal_step_workspace_bytes(B, H, W)


def test_a_cached_workspace_only_grows():
    from mal_amd import step
    dev = torch.device(DEV)
    key = (B, H + 2, W, 3)  # (a shape no other test uses)
    first = step.byte_workspace("multiscale", dev, 1000, *key)
    assert first.numel() >= 1000 and first.dtype == torch.uint8 and first.device == dev
    assert step.byte_workspace("multiscale", dev, 500, *key) is first
    assert step.byte_workspace("multiscale", dev, 1000, *key) is first
    larger = step.byte_workspace("multiscale", dev, 2000, *key)
    assert larger is not first and larger.numel() >= 2000
    assert step.byte_workspace("multiscale", dev, 1000, *key) is larger


class _Step:
    """forward and backward of loss_step on one batch, apart"""

    def __init__(self, seed):
        from mal_amd import trainer
        dev = torch.device(DEV)
        b = make_batch(B, H, W, seed=seed)
        self.opt = trainer.default_options(height=H, width=W, batch_size=B)
        self.inputs, self.mono, self.outputs, self.leaves = to_dicts(b, lambda a, t, inv: None, device=dev)
        for f, s in ((-1, "m1"), (1, "p1")):
            self.mono[("axisangle", 0, f)] = self.leaves["axisangle_" + s]
            self.mono[("translation", 0, f)] = self.leaves["translation_" + s]
        self.noise = torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(seed)).to(dev)

    def forward(self):
        from mal_amd import step
        for t in self.leaves.values():
            t.grad = None
        losses, _, _ = step.loss_step(self.opt, self.inputs, dict(self.mono), dict(self.outputs), noise=self.noise, want_maps=False)
        self.loss = losses["loss"]

    def backward(self):
        self.loss.backward()
        torch.cuda.synchronize()
        return {k: t.grad.clone() for k, t in self.leaves.items()}


def test_two_steps_in_flight_keep_their_maps_apart_under_two_slots_and_are_refused_without():
    from mal_amd import step
    a, b = _Step(11), _Step(12)
    alone = []
    for s in (a, b):
        s.forward()
        alone.append(s.backward())
    assert any(not torch.equal(alone[0][k], alone[1][k]) for k in alone[0])  # two different steps
    with step.workspace_slot(0):
        a.forward()
    with step.workspace_slot(1):
        b.forward()
    got_b = b.backward()
    got_a = a.backward()
    for got, ref in ((got_a, alone[0]), (got_b, alone[1])):
        assert set(got) == set(ref)
        for k in ref:
            assert torch.isfinite(got[k]).all() and torch.equal(got[k], ref[k]), k
    a.forward()
    b.forward()  # the same workspace: a's maps are gone
    b.backward()
    with pytest.raises(L.MalError, match="workspace was reused by a later forward"):
        a.backward()
