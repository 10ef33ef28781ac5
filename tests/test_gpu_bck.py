"""Backward convolution (BckConv: bh_conv2d_bck_nchw and its three separate entry points, bh_bck.hip).

Reference: numpy float64, a loop over the filter taps that adds only true terms (a tap outside the
image or the output contributes nothing, not a zero product), with the sum of the terms' magnitudes
alongside. Inputs are uniform in [-5, 5) (gen_data mode 5's range) from a seeded generator; the three
outputs are filled with NaN before every call, so an element a kernel does not write fails.

Bars, per shape and output: no NaN left; the forward bars of test_gpu_conv.py (max|d| / max(1, max|ref|)
<= 1e-4, rel-L2 <= 1e-5); element-wise |d| <= gamma_{n+64} * sum|terms| (Higham, any summation order;
n = OC*KY*KX for the input gradient, B*OH*OW for the filter and bias gradients; + 64 for the products,
a split combine and the rounding of the reference), or min_sig_mag_rel_diff <= 2e-3 where the stride-1
route runs a Winograd kernel.

The NaN test places its NaN on an out_grad element whose window lies wholly inside the image. For
the input gradient the NaN set is exact anywhere (out_grad is the masked operand: a missed load is a
0 and 0 * filter = 0). For the filter gradient out_grad is the UNmasked operand of a GEMM row: where
the input tap of that element is outside the image the product is NaN * 0 = NaN in any MFMA form,
which the sum over true terms does not contain; only an element without masked taps has the same NaN
set in both. That the input's masked taps are missed loads and not products with zero is what the
in_grad half of the test shows.
"""
import functools

import numpy as np
import pytest

import boda_hip
from boda_hip import ops
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

C = ops.ConvShape
SHAPES = [C(2, 3, 5, 7, 6, 3, 2, 1, 1, 0, 0),        # 0 tiny, KY != KX, nothing a multiple of a tile
          C(3, 16, 13, 13, 40, 3, 3, 1, 1, 1, 1),    # 1 stride-1 padded: the forward route; OC % 32 != 0
          C(2, 33, 9, 11, 35, 1, 1, 1, 1, 0, 0),     # 2 1x1, odd channel counts
          C(1, 4, 6, 6, 5, 1, 1, 1, 1, 1, 1),        # 3 pad > K-1: leaves the forward route (OH = 8)
          C(2, 3, 23, 23, 20, 7, 7, 2, 2, 3, 3),     # 4 7x7 s2 p3 stem; kernel not a multiple of stride
          C(1, 3, 37, 37, 17, 11, 11, 4, 4, 0, 0),   # 5 11x11 s4: rows / columns 35, 36 under no window
          C(2, 8, 12, 10, 12, 5, 5, 2, 2, 2, 2),     # 6 5x5 s2 padded, OH != OW
          C(2, 5, 8, 9, 7, 3, 3, 2, 1, 1, 0),        # 7 sy != sx, py != px
          C(5, 24, 14, 14, 64, 5, 5, 1, 1, 2, 2),    # 8 a listed op; reduction 980
          C(3, 16, 55, 55, 64, 3, 3, 1, 1, 1, 1),    # 9 a listed op; reduction 9075: several splits
          C(20, 96, 27, 27, 33, 1, 1, 1, 1, 0, 0)]   # 10 reduction 14580, 33 x 96 output: many splits
IDS = ["x".join(map(str, s.as_dims())) for s in SHAPES]
U32 = 2.0 ** -24


def gamma(n):
    n = n + 64
    return n * U32 / (1 - n * U32)


def tap_range(n_out, n_in, k, stride, pad):
    """Outputs o with 0 <= o*stride + k - pad < n_in, as (o0, o1, i0); empty: None."""
    o = [x for x in range(n_out) if 0 <= x * stride + k - pad < n_in]
    return (o[0], o[-1] + 1, o[0] * stride + k - pad) if o else None


def ref_bck(i, f, og, s):
    """float64 gradients (in, filts, biases) and the sums of |terms|, true terms only."""
    i = i.reshape(s.B, s.IC, s.H, s.W).astype(np.float64)
    f = f.reshape(s.OC, s.IC, s.KY, s.KX).astype(np.float64)
    og = og.reshape(s.B, s.OC, s.OH, s.OW).astype(np.float64)
    ig, ia = np.zeros_like(i), np.zeros_like(i)
    fg, fa = np.zeros_like(f), np.zeros_like(f)
    for ky in range(s.KY):
        ry = tap_range(s.OH, s.H, ky, s.sy, s.py)
        for kx in range(s.KX):
            rx = tap_range(s.OW, s.W, kx, s.sx, s.px)
            if ry is None or rx is None:
                continue
            g = og[:, :, ry[0]:ry[1], rx[0]:rx[1]]
            ys = slice(ry[2], ry[2] + (ry[1] - ry[0] - 1) * s.sy + 1, s.sy)
            xs = slice(rx[2], rx[2] + (rx[1] - rx[0] - 1) * s.sx + 1, s.sx)
            x = i[:, :, ys, xs]
            fg[:, :, ky, kx] = np.einsum("nohw,nchw->oc", g, x)
            fa[:, :, ky, kx] = np.einsum("nohw,nchw->oc", np.abs(g), np.abs(x))
            ig[:, :, ys, xs] += np.einsum("nohw,oc->nchw", g, f[:, :, ky, kx])
            ia[:, :, ys, xs] += np.einsum("nohw,oc->nchw", np.abs(g), np.abs(f[:, :, ky, kx]))
    return (ig.ravel(), fg.ravel(), og.sum(axis=(0, 2, 3))), (ia.ravel(), fa.ravel(), np.abs(og).sum(axis=(0, 2, 3)))


@functools.lru_cache(maxsize=None)
def case(k):
    """Inputs and reference of SHAPES[k], made once and shared (read-only)."""
    s = SHAPES[k]
    rng = np.random.default_rng(1000 + k)
    i = rng.uniform(-5, 5, s.B * s.IC * s.H * s.W).astype(np.float32)
    f = rng.uniform(-5, 5, s.OC * s.K).astype(np.float32)
    og = rng.uniform(-5, 5, s.B * s.OC * s.OH * s.OW).astype(np.float32)
    ref, mag = ref_bck(i, f, og, s)
    for a in (i, f, og) + ref + mag:
        a.setflags(write=False)
    return i, f, og, ref, mag


class Bufs:
    def __init__(self, dev, s, i, f, og):
        self.dev, self.s = dev, s
        n = (i.size, f.size, og.size, i.size, f.size, s.OC)
        self.i, self.f, self.og, self.ig, self.fg, self.bg = (dev.alloc_floats(x) for x in n)
        self.i.upload(i)
        self.f.upload(f)
        self.og.upload(og)
        self.pk = dev.alloc_floats(boda_hip.conv_bck_filts_packed_floats(s))
        dev.conv_bck_filts_pack(self.f, self.pk, s)

    def nan_fill(self):
        for b in (self.ig, self.fg, self.bg):
            b.upload(np.full(b.nfloats, np.nan, np.float32))

    def outs(self):
        return self.ig.download(), self.fg.download(), self.bg.download()

    def run(self, packed=True, in_grad=True):
        self.nan_fill()
        self.dev.conv_bck(self.i, self.f, self.og, self.ig if in_grad else None, self.fg, self.bg, self.s,
                          packed=self.pk if packed else None)
        return self.outs()

    def free(self):
        for b in (self.i, self.f, self.og, self.ig, self.fg, self.bg, self.pk):
            b.free()


@pytest.fixture
def bufs(dev):
    made = []

    def make(k, og=None):
        i, f, og0 = case(k)[:3]
        made.append(Bufs(dev, SHAPES[k], i, f, og0 if og is None else og))
        return made[-1]
    yield make
    for b in made:
        b.free()


def check(s, name, got, ref, mag, n, wino=False, ok=None):
    if ok is not None:
        got, ref, mag = got[ok], ref[ok], mag[ok]
    assert not np.isnan(got).any(), (s, name, "NaN left in the output")
    nm, rl2, hyb = orc.normalized_errors(ref, got)
    d = np.abs(got.astype(np.float64) - ref)
    lim = gamma(n) * mag
    worst = float((d / np.maximum(lim, 1e-30)).max())
    print("%s %s: norm-max %.3g rel-L2 %.3g hybrid %.3g worst |d|/bound %.3g" % (s.as_dims(), name, nm, rl2, hyb, worst))
    assert nm <= 1e-4 and rl2 <= 1e-5, (s, name, nm, rl2)
    if wino:
        assert hyb <= 2e-3, (s, name, hyb)
    else:
        assert (d <= lim).all(), (s, name, "worst |d| / bound %.3g" % worst)


def check_all(dev, s, outs, ref, mag, ok=(None, None, None)):
    wino = "_wino_" in dev.variant(2, s.as_dims())
    check(s, "in_grad", outs[0], ref[0], mag[0], s.OC * s.KY * s.KX, wino, ok[0])
    check(s, "filts_grad", outs[1], ref[1], mag[1], s.B * s.OH * s.OW, False, ok[1])
    check(s, "biases_grad", outs[2], ref[2], mag[2], s.B * s.OH * s.OW, False, ok[2])


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_bck_gradients(dev, bufs, k):
    s = SHAPES[k]
    ref, mag = case(k)[3:]
    outs = bufs(k).run()
    check_all(dev, s, outs, ref, mag)
    if k == 5:  # rows and columns 35, 36 lie under no window of an 11x11 s4 op over 37: exactly 0
        ig = outs[0].reshape(s.B, s.IC, s.H, s.W)
        unc = np.ones((s.H, s.W), bool)
        unc[:35, :35] = False
        assert unc.sum() * s.B * s.IC == 432
        assert (ig[:, :, unc] == 0).all()


@pytest.mark.parametrize("k", [1, 4, 9], ids=lambda k: IDS[k])
def test_bck_entry_points_agree(dev, bufs, k):
    """Separate calls, no pack, a repeat and in_grad = NULL are bit-identical to the combined call."""
    s = SHAPES[k]
    b = bufs(k)
    ig, fg, bg = b.run()
    for got, exp in zip(b.run(), (ig, fg, bg)):  # a second call
        np.testing.assert_array_equal(got, exp)
    for got, exp in zip(b.run(packed=False), (ig, fg, bg)):  # the pack made inside the call
        np.testing.assert_array_equal(got, exp)
    b.nan_fill()
    dev.conv_bck_in(b.f, b.og, b.ig, s, packed=b.pk)
    dev.conv_bck_filts(b.i, b.og, b.fg, s)
    dev.conv_bck_biases(b.og, b.bg, s)
    for got, exp in zip(b.outs(), (ig, fg, bg)):
        np.testing.assert_array_equal(got, exp)
    b.nan_fill()
    dev.conv_bck_in(b.f, b.og, b.ig, s)
    np.testing.assert_array_equal(b.ig.download(), ig)
    got = b.run(in_grad=False)
    assert np.isnan(got[0]).all()  # untouched
    np.testing.assert_array_equal(got[1], fg)
    np.testing.assert_array_equal(got[2], bg)


def test_bck_variants(dev):
    assert dev.variant(2, SHAPES[1].as_dims()).startswith("bck_in_fwd:")
    assert dev.variant(2, SHAPES[1].as_dims()) == boda_hip.variant_name(2, SHAPES[1].as_dims())
    for k in range(3, 8):
        assert dev.variant(2, SHAPES[k].as_dims()).startswith("mfma32_bcki_"), k
    for k in range(len(SHAPES)):
        assert dev.variant(3, SHAPES[k].as_dims()).startswith("mfma32_bckf_"), k
    # the heuristic reaches every instantiation on these shapes
    names2, names3 = boda_hip.tune_cfg_names(2), boda_hip.tune_cfg_names(3)
    assert names2[-1] == "ref64" and names3[-1] == "ref64" and len(names2) <= 5 and len(names3) <= 5
    seen2 = {dev.variant(2, s.as_dims()) for s in SHAPES}
    seen3 = {dev.variant(3, s.as_dims()).rsplit("_s", 1)[0] for s in SHAPES}
    assert {"mfma32_bcki_" + n for n in names2[:-1]} <= seen2
    assert {"mfma32_bckf_" + n for n in names3[:-1]} == seen3
    assert int(dev.variant(3, SHAPES[9].as_dims()).rsplit("_s", 1)[1]) > 4
    assert int(dev.variant(3, SHAPES[10].as_dims()).rsplit("_s", 1)[1]) > 16


@pytest.mark.parametrize("k", [1, 3, 5, 7], ids=lambda k: IDS[k])
def test_bck_forced_configs(dev, bufs, k):
    """Every configuration of op 2 / op 3 forced on shapes of either route (and other split counts)
    meets the same bars; ref64 is held to fp32 rounding of the double reference."""
    s = SHAPES[k]
    ref, mag = case(k)[3:]
    b = bufs(k)
    names2, names3 = boda_hip.tune_cfg_names(2), boda_hip.tune_cfg_names(3)
    try:
        for c in range(len(names2) - 1):
            dev.tune_set(2, c, 0)
            dev.tune_set(3, c % (len(names3) - 1), 3)
            assert dev.variant(2, s.as_dims()) == "mfma32_bcki_" + names2[c]
            assert dev.variant(3, s.as_dims()).startswith("mfma32_bckf_" + names3[c % (len(names3) - 1)] + "_s")
            check_all(dev, s, b.run(), ref, mag)
        dev.tune_set(2, names2.index("ref64"), 0)
        dev.tune_set(3, names3.index("ref64"), 0)
        assert dev.variant(2, s.as_dims()) == "ref64_bck_in_double"
        assert dev.variant(3, s.as_dims()) == "ref64_bck_filts_double"
        outs = b.run()
        for got, r in zip(outs, ref):
            assert not np.isnan(got).any()
            assert orc.normalized_errors(r, got)[2] <= 1e-6
    finally:
        dev.tune_set(2, -1, 0)
        dev.tune_set(3, -1, 0)


def test_gen_bck_out_grad(dev):
    """BH_GEN_BCK_OUT_GRAD: gen_data_Convolution_in's modes (2: x, 5: hash in [-5, 5)), its own seed."""
    d = [2, 3, 5, 7]
    a, b = dev.alloc_floats(210), dev.alloc_floats(210)
    dev.gen_data(boda_hip.GEN_BCK_OUT_GRAD, a, d, 2)
    np.testing.assert_array_equal(a.download().reshape(d), np.broadcast_to(np.arange(7, dtype=np.float32), d))
    dev.gen_data(boda_hip.GEN_BCK_OUT_GRAD, a, d, 5)
    dev.gen_data(boda_hip.GEN_CONV_IN, b, d, 5)
    x, y = a.download(), b.download()
    assert (x >= -5).all() and (x < 5).all() and len(np.unique(x)) > 200 and (x != y).sum() > 200
    a.free()
    b.free()


@pytest.mark.parametrize("k", [4, 9], ids=lambda k: IDS[k])
def test_bck_nan_set(dev, bufs, k):
    """One NaN in out_grad (an element whose window is wholly in the image, see the module docstring):
    the NaN sets of in_grad and filts_grad are the reference's, every other element meets the bars."""
    s = SHAPES[k]
    i, f, og = case(k)[:3]
    og = og.copy()
    n, oc, oy, ox = s.B - 1, s.OC // 2, s.OH // 2, s.OW // 2
    assert 0 <= oy * s.sy - s.py and oy * s.sy - s.py + s.KY <= s.H and 0 <= ox * s.sx - s.px and ox * s.sx - s.px + s.KX <= s.W
    og[((n * s.OC + oc) * s.OH + oy) * s.OW + ox] = np.nan
    ref, mag = ref_bck(i, f, og, s)
    outs = bufs(k, og).run()
    assert np.isnan(ref[0]).any() and np.isnan(ref[1]).any()
    np.testing.assert_array_equal(np.isnan(outs[0]), np.isnan(ref[0]))
    np.testing.assert_array_equal(np.isnan(outs[1]), np.isnan(ref[1]))
    np.testing.assert_array_equal(np.isnan(outs[2]), np.isnan(ref[2]))
    check_all(dev, s, outs, ref, mag, ok=tuple(~np.isnan(r) for r in ref))
