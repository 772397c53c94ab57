"""Exact checks of the v2 conv forward kernel (k_conv_fwd2) alone: tie-breaking of the conv2 max-pool,
every conv2 operand position (one-tap weights), and that no store leaves its buffer.

A block is one image x one co-half, so B = 1 and B = 3 exercise everything a larger batch does.
All comparisons are torch.equal over whole tensors.
"""
import pytest
import torch

from pytorch_distributed_example_amd._ext import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda"
F_SENTINEL = -12345.0
B_SENTINEL = 0xAB
BATCHES = [1, 3]


def _inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 784, generator=g)
    w1 = torch.randn(20, 1, 5, 5, generator=g) * 0.2
    b1 = torch.randn(20, generator=g) * 0.1
    b2 = torch.randn(50, generator=g) * 0.5
    return x, w1, b1, b2


class _Run:
    """One launch of lenet_conv_fwd2 with every output backed by a buffer one image longer than B,
    the extra image pre-filled with a sentinel."""

    def __init__(self, B, x, w1, b1, w2, b2, zero_n=0):
        K = kernels()
        self.B = B
        self.bufs = {}
        views = {}
        for name, per, dt, sent in (("P1", 2880, torch.float32, F_SENTINEL), ("A1", 2880, torch.uint8, B_SENTINEL),
                                    ("P2", 800, torch.float32, F_SENTINEL), ("A2", 800, torch.uint8, B_SENTINEL)):
            buf = torch.full(((B + 1) * per,), sent, dtype=dt, device=DEV)
            self.bufs[name] = (buf, per, sent)
            views[name] = buf[: B * per]
        zero = None
        if zero_n:
            self.zbuf = torch.full((zero_n + 1,), F_SENTINEL, device=DEV)
            zero = self.zbuf[:zero_n]
        Wp = torch.zeros(2 * 72 * 256, device=DEV)
        K.lenet_pack_w2_v2(w2.to(DEV).contiguous(), Wp)
        K.lenet_conv_fwd2(x.to(DEV).contiguous(), B, w1.to(DEV).contiguous(), b1.to(DEV), Wp, b2.to(DEV),
                          views["P1"], views["A1"], views["P2"], views["A2"], zero)
        torch.cuda.synchronize()
        self.P1 = views["P1"].cpu().view(B, 20, 12, 12)
        self.A1 = views["A1"].cpu().view(B, 20, 12, 12)
        self.P2 = views["P2"].cpu().view(B, 50, 4, 4)
        self.A2 = views["A2"].cpu().view(B, 50, 4, 4)

    def assert_extra_image_untouched(self):
        for name, (buf, per, sent) in self.bufs.items():
            tail = buf[self.B * per:].cpu()
            assert torch.equal(tail, torch.full_like(tail, sent)), f"{name}: a store landed past image {self.B - 1}"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("bias", [0.5, -0.5])
def test_ties_take_the_first_maximum(B, bias):
    """w2 = 0: all four values of every pooling window are relu(b2): P2 = max(b2, 0), code 0."""
    x, w1, b1, _ = _inputs(B, seed=100 + B)
    r = _Run(B, x, w1, b1, torch.zeros(50, 20, 5, 5), torch.full((50,), bias))
    assert torch.equal(r.P2, torch.full((B, 50, 4, 4), max(bias, 0.0)))
    assert torch.equal(r.A2, torch.zeros(B, 50, 4, 4, dtype=torch.uint8))
    r.assert_extra_image_untouched()


def _one_tap_weight(v):
    """w2[co] = 1 at k' = (kh*5 + kw)*20 + ci = co + 50 v, 0 elsewhere; returns (w2, [(ci, kh, kw)] per co)."""
    w2 = torch.zeros(50, 20, 5, 5)
    taps = []
    for co in range(50):
        k = co + 50 * v
        ci, tap = k % 20, k // 20
        kh, kw = tap // 5, tap % 5
        w2[co, ci, kh, kw] = 1.0
        taps.append((ci, kh, kw))
    return w2, taps


def _expect_one_tap(P1, b2, taps):
    """fp32 on the CPU: conv2 output = the kernel's own P1 window (one exact product, the other 499
    terms are exact zeros) plus the bias, then ReLU and the 2x2 max-pool with ATen's indices."""
    B = P1.shape[0]
    c2 = torch.empty(B, 50, 8, 8)
    for co, (ci, kh, kw) in enumerate(taps):
        c2[:, co] = torch.relu(P1[:, ci, kh:kh + 8, kw:kw + 8] + b2[co])
    p2, idx = torch.nn.functional.max_pool2d(c2, 2, 2, return_indices=True)
    code = (((idx // 8) & 1) * 2 + ((idx % 8) & 1)).to(torch.uint8)
    return p2, code


def _prof_stamps(B, fn):
    """Run fn() with the kernels' phase stamps on; returns (fn's result, conv_fwd stamps [2 B][8])."""
    K = kernels()
    buf = torch.zeros(6 * 4096 * 8, dtype=torch.int64, device=DEV)
    K.lenet_set_prof(buf)
    try:
        out = fn()
    finally:
        K.lenet_set_prof(None)
    torch.cuda.synchronize()
    return out, buf.view(6, 4096, 8)[0, : 2 * B].cpu()


@pytest.mark.parametrize("B", BATCHES)
def test_one_tap_weights_cover_every_operand_position(B):
    """Ten launches put a single 1 at each of the 500 k' positions of each of the 50 channels (co 48 /
    49 and the padded rows of co-tile 3 included): a mis-indexed operand or a changed tie-break fails.
    The v = 0 launch at B = 3 is repeated with phase stamps on (the PROF instantiation)."""
    x, w1, b1, b2 = _inputs(B, seed=200 + B)
    for v in range(10):
        w2, taps = _one_tap_weight(v)
        r = _Run(B, x, w1, b1, w2, b2)
        p2, code = _expect_one_tap(r.P1, b2, taps)
        assert torch.equal(r.P2, p2), f"P2, v = {v}"
        assert torch.equal(r.A2, code), f"A2, v = {v}"
        r.assert_extra_image_untouched()
        if v == 0 and B == 3:
            rp, stamps = _prof_stamps(B, lambda: _Run(B, x, w1, b1, w2, b2))
            assert torch.equal(rp.P1, r.P1) and torch.equal(rp.A1, r.A1)
            assert torch.equal(rp.P2, r.P2) and torch.equal(rp.A2, r.A2)
            rp.assert_extra_image_untouched()
            assert (stamps[:, :6] > 0).all(), "a block left a phase stamp unwritten"
            assert (stamps[:, 1:6] >= stamps[:, 0:5]).all(), "phase stamps out of order"


@pytest.mark.parametrize("B", BATCHES)
def test_zero_range_is_exactly_the_view(B):
    """The gradient-zeroing side job clears exactly the elements of the tensor it is given."""
    x, w1, b1, b2 = _inputs(B, seed=300 + B)
    n = 2 * 512 * B + 301                      # more than one pass of the grid-stride loop, ragged end
    w2, _ = _one_tap_weight(3)
    r = _Run(B, x, w1, b1, w2, b2, zero_n=n)
    z = r.zbuf.cpu()
    assert torch.equal(z[:n], torch.zeros(n))
    assert z[n].item() == F_SENTINEL
    r.assert_extra_image_untouched()
