"""The float64 restatements of bckops_ref.py against torch.autograd, where the two definitions coincide:
whole-window pooling without ties, LRN, cross-entropy with mean over the batch. Run as a program by
test_bckops_cpu.py: torch brings a HIP runtime of its own, and a process that has loaded it no longer finds
the GPU through libboda_hip.so, so torch stays out of the process the GPU tests share. Exits 3 without torch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import bckops_ref as R  # noqa: E402
from oracle import layers as L  # noqa: E402

try:
    import torch
except ImportError:
    sys.exit(3)


def _rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


SPREADING = [(2, 3, 9, 9, 3, 3, 2, 2, 0, 0, 0), (2, 3, 8, 8, 2, 2, 2, 2, 0, 0, 0), (1, 4, 7, 7, 3, 3, 1, 1, 0, 0, 0),
             (2, 3, 9, 9, 3, 3, 2, 2, 0, 0, 1), (2, 5, 6, 6, 6, 6, 1, 1, 0, 0, 1)]
LRN = [(2, 13, 3, 5, 3, 0.5, 0.6, 2.0), (1, 2, 4, 4, 7, 1.0, 1.0, 1.0), (1, 40, 2, 3, 5, 1e-2, 0.75, 1.0)]
SOFTMAX = [(5, 10, 1, 1), (3, 7, 2, 3)]


def spreading(p):
    B, C, H, W, KY, KX, sy, sx, py, px, avg = p
    x = _rand((B, C, H, W), 1)  # random: no window has two equal maxima
    out, yx = L.pool(x, KY, KX, sy, sx, py, px, avg)
    og = _rand(out.shape, 2)
    ref, _, cnt = R.spreading(og, yx, x.shape, KY, KX, sy, sx, py, px, avg)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    f = torch.nn.functional.avg_pool2d if avg else torch.nn.functional.max_pool2d
    to = f(tx, (KY, KX), (sy, sx), (py, px))
    assert tuple(to.shape) == out.shape  # whole windows only: the two size rules coincide
    to.backward(torch.tensor(og, dtype=torch.float64))
    np.testing.assert_allclose(ref, tx.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert cnt.max() <= -(-KY // sy) * -(-KX // sx)


def lrn(p):
    B, C, H, W, ls, alpha, beta, k = p
    x, og = _rand((B, C, H, W), 3), _rand((B, C, H, W), 4)
    out, sb = L.lrn(x, ls, alpha, beta, k)
    ref, mag = R.lrn_bck(x, out, sb, og, ls, alpha, beta)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    to = torch.nn.functional.local_response_norm(tx, ls, float(np.float32(alpha)), float(np.float32(beta)), k)
    to.backward(torch.tensor(og, dtype=torch.float64))
    # out and scale_base are the fp32 forward's (a running sum): 1e-5 of the terms' magnitude
    assert (np.abs(ref - tx.grad.numpy()) <= 1e-5 * mag).all()


def softmax(shape):
    B, C, H, W = shape
    x = _rand(shape, 5) * 3
    label = np.random.default_rng(6).integers(0, C, (B, H, W))
    prob = L.softmax(x)
    g, lpp = R.sm_grad_and_loss(prob, label.astype(np.float32))
    loss = R.sum_loss_over_imgs(lpp)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tl = torch.nn.functional.cross_entropy(tx, torch.tensor(label), reduction="none")  # B x H x W
    tl.mean(dim=0).sum().backward()  # mean over the batch, every pixel's loss counted once
    np.testing.assert_allclose(lpp, tl.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(loss, tl.detach().numpy().mean(axis=0), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g, tx.grad.numpy(), rtol=1e-5, atol=1e-7)


if __name__ == "__main__":
    for f, cases in ((spreading, SPREADING), (lrn, LRN), (softmax, SOFTMAX)):
        for c in cases:
            f(c)
            print("ok", f.__name__, c)
