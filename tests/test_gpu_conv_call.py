"""What one description of a conv call (bh::conv_call) and launch_conv's attempt loop must keep:

  * a table line that routes a shape to a direct-family config built for another kernel / stride is
    served through the fallback (the heuristic's choice), with the bits of a call that was given a
    pack, and with ONE start and ONE stop event across repack + fallback (bh_time_next_call);
    the same config forced with bh_tune_set is BH_UNSUP instead. The table is read once per process,
    so this runs in a fresh child process with BH_TUNE_FILE pointing at a table of its own.
  * the four C-ABI forward entries (_pk, _res, _slab, _pkb) agree bitwise where their semantics
    coincide, and each answers a bad call with the error code it always had.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import boda_hip
from boda_hip import BH_ERR, BH_UNSUP, GEN_CONV_BIASES, GEN_CONV_FILTS, GEN_CONV_IN, ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = ops.ConvShape

# dc7s2x64d2 is a 7x7 stride-2 stem config: neither shape is its kernel. The first falls back to a tile
# kernel (OC <= 32), the second to a ring kernel, which reads the pack the first attempt made.
FALLBACK_SHAPES = (C(1, 16, 12, 12, 16, 3, 3, 1, 1, 1, 1), C(1, 64, 40, 40, 96, 3, 3, 1, 1, 1, 1))

CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(root)r + "/boda-1_amd", %(root)r + "/tests"]
import numpy as np
import boda_hip
from boda_hip import ops
from oracle import oracle as orc
from test_gpu_conv import NORM_TOL, RL2_TOL, abs_terms, assert_elem_bound

names = boda_hip.tune_cfg_names(1)
with boda_hip.Device(0) as dev:
    for dims in %(shapes)r:
        s = ops.ConvShape(*dims)
        assert dev.variant(1, s.as_dims()) == "mfma32_conv_direct_dc7s2x64d2", dev.variant(1, s.as_dims())
        hi, hf, hb = orc.gen_conv(s, 5)
        i, f, b = dev.alloc_floats(hi.size), dev.alloc_floats(hf.size), dev.alloc_floats(hb.size)
        n = s.B * s.OC * s.OH * s.OW
        o1, o2 = dev.alloc_floats(n), dev.alloc_floats(n)
        pk = dev.alloc_floats(boda_hip.conv_filts_packed_floats(s))
        i.upload(hi); f.upload(hf); b.upload(hb)
        dev.conv_filts_pack(f, pk, s)
        dev.conv(i, f, b, o1, s, 1)  # eager once: scratch grown before the timed call
        ev_b, ev_e = dev.time_next_call()
        dev.conv(i, f, b, o1, s, 1)  # no pack: repack, the direct launcher's BH_UNSUP, the fallback
        dev.sync()
        ms = dev.elapsed_ms(ev_b, ev_e)
        print("shape", dims, "elapsed ms", ms)
        assert ms > 0, ms
        dev.conv(i, f, b, o2, s, 1, packed=pk)
        got, got_pk = o1.download(), o2.download()
        assert np.array_equal(got, got_pk)
        ref = orc.conv_ref(hi, hf, hb, s, 1)
        nm, rl2, _ = orc.normalized_errors(ref, got)
        print("shape", dims, "norm-max", nm, "rel-L2", rl2)
        assert nm <= NORM_TOL and rl2 <= RL2_TOL, (nm, rl2)
        assert_elem_bound(ref, got, s, None, abs_terms(hi, hf, hb, s))
        # the same config as an override: BH_UNSUP is the answer, not papered over
        dev.tune_set(1, names.index("dc7s2x64d2"), 0)
        try:
            dev.conv(i, f, b, o1, s, 1)
            raise SystemExit("forced dc7s2x64d2 ran on %%r" %% (dims,))
        except boda_hip.UnsupportedError:
            pass
        finally:
            dev.tune_set(1, -1, 0)
print("child ok")
"""


def test_table_route_to_unsupported_direct_config_falls_back(tmp_path):
    table = tmp_path / "one.tune"
    table.write_text("".join("conv %s cfg=dc7s2x64d2 splits=0 red=i\n" % " ".join(map(str, s.as_dims()))
                             for s in FALLBACK_SHAPES))
    script = tmp_path / "child.py"
    script.write_text(CHILD % {"root": ROOT, "shapes": [tuple(s.as_dims()) for s in FALLBACK_SHAPES]})
    env = dict(os.environ, BH_TUNE_FILE=str(table))
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0 and "child ok" in r.stdout


def code_of(call):
    with pytest.raises(boda_hip.BodaHipError) as e:
        call()
    return e.value.code


def test_abi_entries_agree(dev):
    s = C(2, 32, 7, 9, 40, 1, 1, 1, 1, 0, 0)  # ragged: OH*OW = 63, OC no multiple of a tile
    n, ohw = s.B * s.OC * s.OH * s.OW, s.OH * s.OW
    i, f, b = dev.alloc_floats(s.B * s.IC * s.H * s.W), dev.alloc_floats(s.OC * s.K), dev.alloc_floats(s.OC)
    dev.gen_data(GEN_CONV_IN, i, [s.B, s.IC, s.H, s.W], 5)
    dev.gen_data(GEN_CONV_FILTS, f, [s.OC, s.IC, s.KY, s.KX], 5)
    dev.gen_data(GEN_CONV_BIASES, b, [s.OC], 5)
    pk = dev.alloc_floats(boda_hip.conv_filts_packed_floats(s))
    dev.conv_filts_pack(f, pk, s)
    r = dev.alloc_floats(n)
    r.upload((np.random.default_rng(7).standard_normal(n) * 3).astype(np.float32))
    o = dev.alloc_floats(n)
    wide = dev.alloc_floats(s.B * (s.OC + 8) * ohw)

    def out_of(call):
        o.upload(np.full(n, -7.25, np.float32))
        call()
        return o.download()

    plain = out_of(lambda: dev.conv(i, f, b, o, s, 1))
    np.testing.assert_array_equal(out_of(lambda: dev.conv(i, f, b, o, s, 1, packed=pk)), plain)
    np.testing.assert_array_equal(out_of(lambda: dev.conv_pkb(i, f, None, 0, b, o, s, 1)), plain)
    np.testing.assert_array_equal(out_of(lambda: dev.conv_pkb(i, f, pk, boda_hip.BANKS_ALL, b, o, s, 1)), plain)
    np.testing.assert_array_equal(out_of(lambda: dev.conv_slab(i, f, b, o, s.OC, 0, s, 1)), plain)
    np.testing.assert_array_equal(out_of(lambda: dev.conv_pkb(i, f, None, 0, b, o, s, 1, out_chans_total=s.OC)), plain)
    with_res = out_of(lambda: dev.conv_res(i, f, b, r, o, s, 1))
    assert not np.array_equal(with_res, plain)
    np.testing.assert_array_equal(out_of(lambda: dev.conv_pkb(i, f, None, 0, b, o, s, 1, res=r)), with_res)
    # a slab of a wider tensor: _slab and _pkb write the same bytes, the plain call's, and nothing else
    ctot, ofs = s.OC + 8, 3
    slabs = []
    for call in (lambda: dev.conv_slab(i, f, b, wide, ctot, ofs, s, 1),
                 lambda: dev.conv_pkb(i, f, None, 0, b, wide, s, 1, out_chans_total=ctot, out_chan_ofs=ofs)):
        wide.upload(np.full(s.B * ctot * ohw, -3.5, np.float32))
        call()
        slabs.append(wide.download().reshape(s.B, ctot, ohw))
    np.testing.assert_array_equal(slabs[0], slabs[1])
    np.testing.assert_array_equal(slabs[0][:, ofs:ofs + s.OC], plain.reshape(s.B, s.OC, ohw))
    assert (slabs[0][:, :ofs] == -3.5).all() and (slabs[0][:, ofs + s.OC:] == -3.5).all()

    # ---- error codes, per entry: (shape, tensors) -> the call through each entry
    class Null:
        ptr = None

    def entries(sh, fi=f, with_slab=True):
        e = {"pk": lambda: dev.conv(i, fi, b, o, sh, 1, packed=pk),
             "res": lambda: dev.conv_res(i, fi, b, r, o, sh, 1),
             "pkb": lambda: dev.conv_pkb(i, fi, None, 0, b, o, sh, 1)}
        if with_slab:
            e["slab"] = lambda: dev.conv_slab(i, fi, b, wide, ctot, ofs, sh, 1)
        return e

    for name, call in entries(s, fi=Null).items():
        assert code_of(call) == BH_ERR, name  # a null tensor
    zero_stride = C(2, 32, 7, 9, 40, 1, 1, 0, 1, 0, 0)
    small = C(2, 32, 7, 9, 40, 11, 11, 1, 1, 1, 1)  # 7 + 2 < 11: the padded input holds no window
    for bad in (zero_stride, small):
        for name, call in entries(bad).items():
            assert code_of(call) == BH_UNSUP, (name, bad)
    # the shape checks come before the slab checks
    assert code_of(lambda: dev.conv_slab(i, f, b, wide, ctot, ctot, small, 1)) == BH_UNSUP
    assert code_of(lambda: dev.conv_pkb(i, f, None, 0, b, wide, small, 1, out_chans_total=ctot, out_chan_ofs=ctot)) == BH_UNSUP
    # a slab past the tensor's channels (for _slab a total of 0 holds no slab at all)
    assert code_of(lambda: dev.conv_slab(i, f, b, wide, ctot, ctot - s.OC + 1, s, 1)) == BH_ERR
    assert code_of(lambda: dev.conv_slab(i, f, b, wide, 0, 0, s, 1)) == BH_ERR
    assert code_of(lambda: dev.conv_pkb(i, f, None, 0, b, wide, s, 1, out_chans_total=ctot, out_chan_ofs=ctot - s.OC + 1)) == BH_ERR
    assert code_of(lambda: dev.conv_pkb(i, f, None, 0, b, o, s, 1, out_chan_ofs=1)) == BH_ERR  # a total of 0 means OC
    # a residual together with a slab; the range check is reported first
    assert code_of(lambda: dev.conv_pkb(i, f, None, 0, b, wide, s, 1, res=r, out_chans_total=ctot)) == BH_ERR
    with pytest.raises(boda_hip.BodaHipError, match="out of range"):
        dev.conv_pkb(i, f, None, 0, b, wide, s, 1, res=r, out_chans_total=ctot, out_chan_ofs=ctot)
    with pytest.raises(boda_hip.BodaHipError, match="residual and channel slab"):
        dev.conv_pkb(i, f, None, 0, b, wide, s, 1, res=r, out_chans_total=ctot, out_chan_ofs=ofs)
    # every rejected call left the output alone
    np.testing.assert_array_equal(out_of(lambda: None), np.full(n, -7.25, np.float32))
    for x in (i, f, b, pk, r, o, wide):
        x.free()
