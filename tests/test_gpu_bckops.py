"""GPU parity of the backward ops of the non-conv layers (bh_bckops.hip, through the C-ABI) against the
float64 restatements in tests/bckops_ref.py, on inputs made by the device's own forward kernels.

Bars (include/boda_hip.h and DESIGN.md 8c):
* Spreading: |got - ref64| <= T * 2^-23 * sum|terms|, T the element's term count (an fp32 sum of T
  terms); form 1 (ref64) within 2^-23 relative.
* BckLRN: 4e-6 * (|first term| + |second term's factors summed in absolute value|): the 2e-6 bar of
  the device's scale^-beta (tests/test_gpu_layers.py) plus the rounding of <= 11 fp32 terms and two
  divisions.
* ZeroIfNonPos, Reduce: bit-exact.
* Softmax with loss: gradient rtol 1e-6; loss rtol 2e-6 + atol 1e-7 (the softmax bar plus a device log).
Every production form is run twice and must give identical bits."""
import numpy as np
import pytest

import bckops_ref as R
import boda_hip
from oracle import layers as L

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23


def _up(dev, x):
    b = dev.alloc_floats(x.size)
    b.upload(np.ascontiguousarray(x, dtype=np.float32))
    return b


def _rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _twice(run, out, shape):
    """run() twice into device buffer out: the two results, bit-identical, reshaped."""
    run()
    a = out.download().copy()
    out.upload(np.full(a.size, 7.0, np.float32))  # every element must be written again
    run()
    b = out.download()
    np.testing.assert_array_equal(_bits(a), _bits(b))
    return a.reshape(shape)


def _free(*bufs):
    for b in bufs:
        b.free()


# ---- Spreading
SPREADS = [  # B, C, H, W, KY, KX, sy, sx, py, px, avg, input
    (1, 3, 5, 5, 4, 4, 3, 3, 2, 2, 0, "rand"),     # partial windows at both ends
    (2, 5, 13, 13, 3, 3, 2, 2, 0, 0, 0, "rand"),   # the ceil rule; compile-time 3x3 s2
    (2, 6, 7, 7, 3, 3, 1, 1, 1, 1, 0, "const"),    # all ties, overlapping windows; compile-time 3x3 s1
    (1, 2, 9, 9, 2, 2, 3, 3, 0, 0, 0, "rand"),     # pixels under no window give 0
    (1, 2, 6, 130, 3, 3, 2, 2, 0, 0, 0, "rand"),   # rows wider than a wave
    (2, 3, 8, 10, 2, 2, 2, 2, 0, 0, 0, "rand"),    # compile-time 2x2 s2
    (2, 7, 9, 11, 3, 2, 2, 3, 1, 1, 1, "rand"),    # truncated-window divisors
    (2, 7, 6, 6, 6, 6, 1, 1, 0, 0, 1, "rand"),     # global pooling
    (2, 4, 7, 7, 3, 3, 1, 1, 1, 1, 1, "rand"),     # compile-time 3x3 s1, padded average
]


@pytest.mark.parametrize("p", SPREADS, ids=lambda p: "x".join(map(str, p)))
def test_spreading(dev, p):
    B, C, H, W, KY, KX, sy, sx, py, px, avg, kind = p
    x = _rand((B, C, H, W), 11) if kind == "rand" else np.full((B, C, H, W), 1.5, np.float32)
    OH, OW = boda_hip.pool_out_size(H, KY, sy, py), boda_hip.pool_out_size(W, KX, sx, px)
    og = _rand((B, C, OH, OW), 12)
    dx, do, da = _up(dev, x), dev.alloc_floats(og.size), dev.alloc_floats(og.size)
    dev.pool(dx, do, B, C, H, W, KY, KX, sy, sx, py, px, avg, out_in_yx=da)
    yx = da.download().reshape(og.shape)
    dg, di = _up(dev, og), dev.alloc_floats(x.size)
    ref, aref, cnt = R.spreading(og, yx, x.shape, KY, KX, sy, sx, py, px, avg)
    got = _twice(lambda: dev.spreading(dg, None if avg else da, di, B, C, H, W, KY, KX, sy, sx, py, px, avg), di,
                 x.shape)
    err = np.abs(got.astype(np.float64) - ref)
    print("spreading max err / bar:", float((err / np.maximum(cnt * EPS * aref, 1e-300)).max()))
    assert (err <= cnt * EPS * aref).all()
    if not avg and kind == "rand":
        assert (got[cnt == 0] == 0).all()
    dev.spreading(dg, None if avg else da, di, B, C, H, W, KY, KX, sy, sx, py, px, avg, form=1)
    got64 = di.download().reshape(x.shape).astype(np.float64)
    assert (np.abs(got64 - ref) <= EPS * np.abs(ref)).all()
    _free(dx, do, da, dg, di)


def test_spreading_uncovered_pixels_are_zero(dev):
    B, C, H, W = 1, 2, 9, 9  # k2 s3: every third row and column lies between windows
    og = np.ones((B, C, 4, 4), np.float32)
    assert boda_hip.pool_out_size(H, 2, 3, 0) == 4
    dx, do, da = _up(dev, _rand((B, C, H, W), 1)), dev.alloc_floats(og.size), dev.alloc_floats(og.size)
    dev.pool(dx, do, B, C, H, W, 2, 2, 3, 3, 0, 0, 0, out_in_yx=da)
    dg, di = _up(dev, og), _up(dev, np.full((B, C, H, W), 9.0, np.float32))
    dev.spreading(dg, da, di, B, C, H, W, 2, 2, 3, 3, 0, 0, 0)
    got = di.download().reshape(B, C, H, W)
    assert (got[:, :, 2::3, :] == 0).all() and (got[:, :, :, 2::3] == 0).all()
    # each window's gradient lands on exactly one pixel (the fourth row and column of windows start
    # past the image and have none)
    assert got.sum() == B * C * 3 * 3
    _free(dx, do, da, dg, di)


@pytest.mark.parametrize("form", [0, 1])
def test_spreading_no_winner_gives_zeros(dev, form):
    B, C, H, W = 2, 3, 7, 7
    og = _rand((B, C, 3, 3), 5)
    dg, da = _up(dev, og), _up(dev, np.full(og.shape, -1.0, np.float32))
    di = _up(dev, np.full((B, C, H, W), 9.0, np.float32))
    dev.spreading(dg, da, di, B, C, H, W, 3, 3, 2, 2, 0, 0, 0, form=form)
    assert (di.download() == 0).all()
    _free(dg, da, di)


def test_spreading_rejects(dev):
    b = dev.alloc_floats(64)
    with pytest.raises(boda_hip.UnsupportedError):
        dev.spreading(b, b, b, 1, 1, 0, 4, 2, 2, 2, 2, 0, 0, 0)
    with pytest.raises(boda_hip.UnsupportedError):
        dev.spreading(b, b, b, 1, 1, 4, 4, 2, 2, 2, 2, 0, 0, 0, form=2)
    with pytest.raises(boda_hip.UnsupportedError):  # out_in_yx is a float: planes above 2^24 pixels are refused
        dev.spreading(b, b, b, 1, 1, 4097, 4096, 2, 2, 2, 2, 0, 0, 0)
    with pytest.raises(boda_hip.BodaHipError) as e:
        dev.spreading(b, None, b, 1, 1, 4, 4, 2, 2, 2, 2, 0, 0, 0)  # max needs out_in_yx
    assert e.value.code == boda_hip.BH_ERR
    b.free()


# ---- BckLRN
LRNS = [  # B, C, H, W, local_size, alpha, beta, k
    (2, 13, 3, 5, 3, 0.5, 0.6, 2.0),
    (1, 2, 4, 4, 7, 1.0, 1.0, 1.0),       # C < local_size
    (1, 300, 2, 3, 5, 1e-4, 0.75, 1.0),   # many channel chunks per pixel
    (2, 96, 9, 9, 5, 1e-4, 0.75, 1.0),
    (1, 24, 3, 3, 11, 1e-2, 0.75, 1.0),   # the widest window
]


@pytest.mark.parametrize("p", LRNS, ids=lambda p: "x".join(map(str, p[:5])))
def test_lrn_bck(dev, p):
    B, C, H, W, ls, alpha, beta, k = p
    x = _rand((B, C, H, W), 21) * 2
    og = _rand((B, C, H, W), 22)
    dx, do, ds = _up(dev, x), dev.alloc_floats(x.size), dev.alloc_floats(x.size)
    dev.lrn(dx, do, B, C, H, W, ls, alpha, beta, k, out_scale_base=ds)
    out, sb = do.download().reshape(x.shape), ds.download().reshape(x.shape)
    dg, di = _up(dev, og), dev.alloc_floats(x.size)
    ref, mag = R.lrn_bck(x, out, sb, og, ls, alpha, beta)
    got = _twice(lambda: dev.lrn_bck(dx, do, ds, dg, di, B, C, H, W, ls, alpha, beta, k), di, x.shape)
    err = np.abs(got.astype(np.float64) - ref)
    print("lrn_bck max err / magnitude:", float((err / mag).max()))
    assert (err <= 4e-6 * mag).all()
    dev.lrn_bck(dx, do, ds, dg, di, B, C, H, W, ls, alpha, beta, k, form=1)
    err64 = np.abs(di.download().reshape(x.shape).astype(np.float64) - ref)
    assert (err64 <= EPS * mag).all()
    _free(dx, do, ds, dg, di)


def test_lrn_bck_rejects(dev):
    b = dev.alloc_floats(16)
    with pytest.raises(boda_hip.UnsupportedError):
        dev.lrn_bck(b, b, b, b, b, 1, 4, 2, 2, 4, 1.0, 1.0, 1.0)  # even window
    with pytest.raises(boda_hip.UnsupportedError):
        dev.lrn_bck(b, b, b, b, b, 1, 4, 2, 2, 13, 1.0, 1.0, 1.0)
    with pytest.raises(boda_hip.UnsupportedError):
        dev.lrn_bck(b, b, b, b, b, 1, 0, 2, 2, 3, 1.0, 1.0, 1.0)
    b.free()


# ---- ZeroIfNonPos
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000, 4097])
def test_zero_if_non_pos(dev, n, inplace, form):
    x, cond = _rand((n,), 31), _rand((n,), 32)
    special = np.array([0.0, -0.0, np.nan, -1.0, 2.0], np.float32)
    cond[:min(n, 5)] = special[:min(n, 5)]
    if n >= 1000:
        cond[n - 5:] = special            # in the element tail too
        x[n - 4] = np.nan                 # NaN in under cond <= 0 gives 0
        x[7] = np.nan                     # NaN in under whatever cond[7] is: a select passes it or zeroes it
    x[0] = np.nan                         # cond[0] == 0
    ref = R.zero_if_non_pos(x, cond)
    dx, dc = _up(dev, x), _up(dev, cond)
    do = dx if inplace else _up(dev, np.full(n, 7.0, np.float32))
    dev.zero_if_non_pos(dx, dc, do, n, form=form)
    got = do.download()
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    assert got[0] == 0
    if not inplace:  # a second run gives the same bits
        dev.zero_if_non_pos(dx, dc, do, n, form=form)
        np.testing.assert_array_equal(_bits(do.download()), _bits(got))
        do.free()
    _free(dx, dc)


# ---- Reduce
@pytest.mark.parametrize("n", [1, 5, 4099])
@pytest.mark.parametrize("n_ins", [1, 2, 4, 8])
def test_reduce(dev, n_ins, n):
    ins = [_rand((n,), 40 + k) * 10.0 ** (k % 3) for k in range(n_ins)]
    ins[0][0] = -0.0
    bufs = [_up(dev, v) for v in ins]
    do = dev.alloc_floats(n)
    got = _twice(lambda: dev.reduce_sum(bufs, do, n), do, (n,))
    np.testing.assert_array_equal(_bits(got), _bits(R.reduce_sum_f32(ins)))
    dev.reduce_sum(bufs, do, n, form=1)
    ref64 = np.zeros(n, np.float64)
    for v in ins:
        ref64 += v
    np.testing.assert_array_equal(_bits(do.download()), _bits(ref64.astype(np.float32)))
    _free(do, *bufs)


def test_reduce_rejects_nine_inputs(dev):
    b = dev.alloc_floats(8)
    with pytest.raises(boda_hip.UnsupportedError):
        dev.reduce_sum([b] * 9, b, 8)
    with pytest.raises(boda_hip.UnsupportedError):
        dev.reduce_sum([], b, 8)
    b.free()


# ---- SoftmaxWithLoss
def _labels(B, C, H, W, seed):
    return np.random.default_rng(seed).integers(0, C, (B, H, W)).astype(np.float32)


@pytest.mark.parametrize("shape", [(1, 1000, 1, 1), (5, 10, 1, 1), (3, 7, 2, 3), (2, 5, 9, 9)])
def test_softmax_with_loss(dev, shape):
    B, C, H, W = shape
    x, label = _rand(shape, 51) * 3, _labels(B, C, H, W, 52)
    dx, dl = _up(dev, x), _up(dev, label)
    dp, dg, dlp, dls = (dev.alloc_floats(n) for n in (x.size, x.size, B * H * W, H * W))
    # the three entries in turn ...
    dev.softmax(dx, dp, B, C, H, W)
    prob = dp.download().reshape(shape)
    g = _twice(lambda: dev.sm_grad_and_loss(dp, dl, dg, dlp, B, C, H, W), dg, shape)
    lpp = dlp.download().reshape(B, H, W)
    loss = _twice(lambda: dev.sum_loss_over_imgs(dlp, dls, B, H * W), dls, (H, W))
    rg, rlpp = R.sm_grad_and_loss(prob, label)
    np.testing.assert_allclose(g, rg, rtol=1e-6, atol=0)
    np.testing.assert_allclose(lpp, rlpp, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(loss, R.sum_loss_over_imgs(lpp), rtol=2e-6, atol=1e-7)
    # ... the loss is softmax cross-entropy of the inputs, to the softmax bar plus a log
    ref_prob = L.softmax(x).astype(np.float64)
    ref_lpp = -np.log(np.take_along_axis(ref_prob, label.astype(np.int64)[:, None], axis=1)[:, 0])
    np.testing.assert_allclose(lpp, ref_lpp, rtol=2e-6, atol=2e-6 + 1e-7)  # d(-log p) = dp / p: relative 2e-6 of p
    # ... and the one-call entry gives the same bits
    dp2, dg2, dlp2, dls2 = (dev.alloc_floats(n) for n in (x.size, x.size, B * H * W, H * W))
    dev.softmax_with_loss(dx, dl, dp2, dg2, dlp2, dls2, B, C, H, W)
    for a, b in ((dp, dp2), (dg, dg2), (dlp, dlp2), (dls, dls2)):
        np.testing.assert_array_equal(_bits(a.download()), _bits(b.download()))
    # ref64 form
    dev.sm_grad_and_loss(dp, dl, dg2, dlp2, B, C, H, W, form=1)
    np.testing.assert_allclose(dg2.download().reshape(shape), rg, rtol=EPS, atol=0)
    np.testing.assert_allclose(dlp2.download().reshape(B, H, W), rlpp, rtol=EPS, atol=0)
    dev.sum_loss_over_imgs(dlp, dls2, B, H * W, form=1)
    np.testing.assert_allclose(dls2.download().reshape(H, W), R.sum_loss_over_imgs(lpp), rtol=EPS, atol=0)
    _free(dx, dl, dp, dg, dlp, dls, dp2, dg2, dlp2, dls2)


def test_sm_grad_zero_prob_and_bad_labels(dev):
    B, C, H, W = 3, 7, 2, 3
    prob = np.abs(_rand((B, C, H, W), 61)) + 0.01
    label = _labels(B, C, H, W, 62)
    prob[0, int(label[0, 0, 0]), 0, 0] = 0.0   # a prob of exactly 0 at the label: a finite loss
    label[1, 1, 2] = C                          # out of range
    label[2, 0, 1] = -3.0
    label[2, 1, 0] = np.nan
    bad = [(1, 1, 2), (2, 0, 1), (2, 1, 0)]
    dp, dl = _up(dev, prob), _up(dev, label)
    dg, dlp = dev.alloc_floats(prob.size), dev.alloc_floats(B * H * W)
    dev.sm_grad_and_loss(dp, dl, dg, dlp, B, C, H, W)
    g, lpp = dg.download().reshape(prob.shape), dlp.download().reshape(B, H, W)
    rg, rlpp = R.sm_grad_and_loss(prob, label)
    np.testing.assert_allclose(lpp[0, 0, 0], -np.log(R.FLT_MIN), rtol=2e-6)
    for n, y, x in bad:
        assert np.isnan(lpp[n, y, x]) and np.isnan(g[n, :, y, x]).all()
    ok = ~np.isnan(rlpp)
    assert ok.sum() == B * H * W - len(bad)
    np.testing.assert_allclose(lpp[ok], rlpp[ok], rtol=2e-6, atol=1e-7)
    okg = np.broadcast_to(ok[:, None], prob.shape)
    np.testing.assert_allclose(g[okg], rg[okg], rtol=1e-6, atol=0)   # nothing else is disturbed
    _free(dp, dl, dg, dlp)


def test_softmax_with_loss_rejects(dev):
    b = dev.alloc_floats(16)
    with pytest.raises(boda_hip.UnsupportedError):
        dev.sm_grad_and_loss(b, b, b, b, 0, 4, 1, 1)
    with pytest.raises(boda_hip.UnsupportedError):
        dev.sum_loss_over_imgs(b, b, 2, 0)
    with pytest.raises(boda_hip.UnsupportedError):
        dev.softmax_with_loss(b, b, b, b, b, b, 2, 4, 1, 1, form=3)
    b.free()
