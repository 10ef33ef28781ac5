"""CPU restatements (numpy, float64 accumulation from the fp32 inputs) of the backward ops of
boda-1_amd/csrc/bh_bckops.hip, as include/boda_hip.h defines them. Test infrastructure only: shared by
tests/test_bckops_cpu.py (which cross-checks them against torch.autograd where the definitions
coincide) and tests/test_gpu_bckops.py (which holds the kernels to them).

Each sum-shaped restatement returns, next to the float64 result, what the error bar of an fp32
summation needs: the sum of the terms' absolute values and the per-element term count."""
import numpy as np

from oracle import layers as L

F64 = np.float64
FLT_MIN = float(np.finfo(np.float32).tiny)
EPS = 2.0 ** -23


def spreading(og, out_in_yx, in_shape, KY, KX, sy, sx, py, px, avg):
    """in_grad of Pooling: (sum, sum of |terms|, term count), each B x C x H x W. max: a covering
    window contributes out_grad iff its out_in_yx names the pixel; avg: out_grad / (the window's
    in-image tap count)."""
    B, C, H, W = in_shape
    OH, OW = L.pool_out_sz(H, KY, sy, py), L.pool_out_sz(W, KX, sx, px)
    assert og.shape == (B, C, OH, OW)
    s = np.zeros(in_shape, F64)
    a = np.zeros(in_shape, F64)
    cnt = np.zeros(in_shape, np.int64)
    g = og.astype(F64)
    for oy in range(OH):
        y0, y1 = max(0, oy * sy - py), min(H, oy * sy - py + KY)
        for ox in range(OW):
            x0, x1 = max(0, ox * sx - px), min(W, ox * sx - px + KX)
            if y1 <= y0 or x1 <= x0:
                continue
            if avg:
                t = g[:, :, oy, ox] / float((y1 - y0) * (x1 - x0))
                s[:, :, y0:y1, x0:x1] += t[:, :, None, None]
                a[:, :, y0:y1, x0:x1] += np.abs(t)[:, :, None, None]
                cnt[:, :, y0:y1, x0:x1] += 1
            else:
                me = (np.arange(y0, y1)[:, None] * W + np.arange(x0, x1)[None, :]).astype(np.float32)
                hit = out_in_yx[:, :, oy, ox][:, :, None, None] == me[None, None]
                t = np.where(hit, g[:, :, oy, ox][:, :, None, None], 0.0)
                s[:, :, y0:y1, x0:x1] += t
                a[:, :, y0:y1, x0:x1] += np.abs(t)
                cnt[:, :, y0:y1, x0:x1] += 1  # every covering window is a term of the fp32 sum (a 0 if no hit)
    return s, a, cnt


def lrn_bck(x, out, sb, og, local_size, alpha, beta):
    """in_grad of LRN: (result, |first term| + |in * coef| * sum of |t| over the window)."""
    x, out, sb, og = (v.astype(F64) for v in (x, out, sb, og))
    C = x.shape[1]
    hls = local_size // 2
    t = og * out / sb
    win = np.zeros_like(t)
    awin = np.zeros_like(t)
    for c in range(C):
        lo, hi = max(0, c - hls), min(C, c + hls + 1)
        win[:, c] = t[:, lo:hi].sum(axis=1)
        awin[:, c] = np.abs(t[:, lo:hi]).sum(axis=1)
    coef = -2.0 * float(np.float32(beta)) * float(np.float32(alpha)) / local_size
    first = og * sb ** -float(np.float32(beta))
    return first + x * coef * win, np.abs(first) + np.abs(x * coef) * awin


def zero_if_non_pos(x, cond):
    return np.where(cond > 0, x, np.float32(0)).astype(np.float32)


def reduce_sum_f32(ins):
    """((0 + ins_0) + ins_1) + ... in fp32, the production kernel's order."""
    acc = np.zeros_like(ins[0], dtype=np.float32)
    for v in ins:
        acc = (acc + v).astype(np.float32)
    return acc


def sm_grad_and_loss(prob, label):
    """(in_grad, loss_per_pel) with per-pixel labels; a label outside [0, C) gives a NaN pixel."""
    B, C, H, W = prob.shape
    p = prob.astype(F64)
    grad = np.empty_like(p)
    lpp = np.empty((B, H, W), F64)
    for n in range(B):
        for y in range(H):
            for x in range(W):
                lab = label[n, y, x]
                if not (lab >= 0 and lab < C):
                    grad[n, :, y, x] = np.nan
                    lpp[n, y, x] = np.nan
                    continue
                l = int(lab)
                onehot = np.zeros(C)
                onehot[l] = 1.0
                grad[n, :, y, x] = (p[n, :, y, x] - onehot) / B
                lpp[n, y, x] = -np.log(max(p[n, l, y, x], FLT_MIN))
    return grad, lpp


def sum_loss_over_imgs(lpp):
    return lpp.astype(F64).sum(axis=0) / lpp.shape[0]
