"""CPU-only checks of the BckConv host side: the op lists' backward ops parse to consistent shapes in
Python and in C++ (boda_hip_ops_prof --dump-ops --types=BckConv) with the same flop / byte model, and the
library names the variants of op 2 (input gradient) / op 3 (filter gradient) and sizes the bck pack
without a device.

op_sigs_full.txt lists 93 BckConv ops with every tensor's dims. op_sigs.txt lists 10 BckConv
SIGNATURES (kern_sz / stride / in_pad only, no tensor dims): they read as ops but have no shape.
"""
import os
import subprocess

import pytest

import boda_hip
from boda_hip import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = os.path.join(ROOT, "tests", "golden", "ops")
BIN = os.path.join(ROOT, "boda-1_amd", "bin", "boda_hip_ops_prof")
FULL = os.path.join(OPS, "op_sigs_full.txt")


def bck_ops():
    return ops.read_ops(FULL, types=("BckConv",))


def test_read_bck_ops():
    full, skipped = bck_ops()
    assert len(full) == 93 and skipped == 493
    sigs, skipped = ops.read_ops(os.path.join(OPS, "op_sigs.txt"), types=("BckConv",))
    assert len(sigs) == 10 and skipped == 80
    # the default types are unchanged
    conv, skipped = ops.read_ops(FULL)
    assert len(conv) == 178 and skipped == 408
    # a signature carries no tensor dims: no shape
    with pytest.raises(ValueError):
        ops.bck_conv_shape(sigs[0])


def test_bck_shapes_consistent():
    fwd = {tuple(ops.conv_shape(o).as_dims()) for o in ops.read_ops(FULL, types=("Convolution",))[0]}
    for op in bck_ops()[0]:
        s = ops.bck_conv_shape(op)
        assert ops.shape_of(op) == s
        assert tuple(op.dims["in_grad_loss"].values()) == (s.B, s.IC, s.H, s.W)
        assert tuple(op.dims["filts_grad_loss"].values()) == (s.OC, s.IC, s.KY, s.KX)
        assert tuple(op.dims["biases_grad_loss"].values()) == (s.OC,)
        assert tuple(op.dims["out_grad_loss"].values()) == (s.B, s.OC, s.OH, s.OW)
        assert tuple(s.as_dims()) in fwd  # every backward op has its forward twin in the list
        assert ops.bck_flops(s) == 2 * s.flops() + s.M * s.N
        assert ops.bck_bytes(s) == 4 * (2 * s.B * s.IC * s.H * s.W + 2 * s.OC * s.K + s.M * s.N + s.OC)


def short_line(line, var="out_grad_loss"):
    """The op line with var one row short."""
    op = ops.parse_op(line)
    d = op.dims[var]
    old = "%s=(%s)" % (var, ",".join("%s=%d" % kv for kv in d.items()))
    assert old in line
    d = dict(d, y=d["y"] - 1)
    return line.replace(old, "%s=(%s)" % (var, ",".join("%s=%d" % kv for kv in d.items())))


@pytest.mark.parametrize("var", ["out_grad_loss", "in_grad_loss", "filts_grad_loss"])
def test_inconsistent_bck_op_raises(tmp_path, var):
    op = [o for o in bck_ops()[0] if o.dims["filts"]["y"] > 1 and o.dims["out_grad_loss"]["y"] > 1][0]
    bad = short_line(op.line, var)
    with pytest.raises(ValueError):
        ops.bck_conv_shape(ops.parse_op(bad))
    fn = tmp_path / "bad.txt"
    fn.write_text(bad + "\n")
    r = subprocess.run([BIN, "--dump-ops=%s" % fn, "--types=BckConv"], capture_output=True, text=True)
    assert r.returncode != 0 and var in r.stderr


def test_cpp_and_python_parse_agree():
    r = subprocess.run([BIN, "--dump-ops=" + FULL, "--types=BckConv"], capture_output=True, text=True, check=True)
    lines = r.stdout.strip().split("\n")
    py, skipped = bck_ops()
    assert lines[-1] == "skipped %d" % skipped
    assert len(lines) - 1 == len(py)
    for l, op in zip(lines, py):
        f = l.split()
        s = ops.bck_conv_shape(op)
        assert f[0] == "BckConv" and [int(x) for x in f[1:12]] == s.as_dims()
        assert float(f[-2]) == ops.bck_flops(s) and float(f[-1]) == ops.bck_bytes(s)
    # both types in one dump, in list order
    r = subprocess.run([BIN, "--dump-ops=" + FULL, "--types=Convolution,BckConv"], capture_output=True, text=True,
                       check=True)
    both = r.stdout.strip().split("\n")
    assert both[-1] == "skipped %d" % (586 - 178 - 93)
    assert [l for l in both if l.startswith("BckConv")] == lines[:-1]


def test_variant_names_without_device():
    assert boda_hip.tune_cfg_names(2)[-1] == "ref64" and boda_hip.tune_cfg_names(3)[-1] == "ref64"
    for op in bck_ops()[0]:
        s = ops.bck_conv_shape(op)
        v2, v3 = boda_hip.variant_name(2, s.as_dims()), boda_hip.variant_name(3, s.as_dims())
        fwd = s.sy == 1 and s.sx == 1 and s.py <= s.KY - 1 and s.px <= s.KX - 1
        assert v2.startswith("bck_in_fwd:" if fwd else "mfma32_bcki_"), (s, v2)
        if fwd:  # the forward conv of out_grad with the transposed bank, at pad K-1-p
            twin = [s.B, s.OC, s.OH, s.OW, s.IC, s.KY, s.KX, 1, 1, s.KY - 1 - s.py, s.KX - 1 - s.px]
            assert v2 == "bck_in_fwd:" + boda_hip.variant_name(1, twin)
        assert v3.startswith("mfma32_bckf_") and int(v3.rsplit("_s", 1)[1]) >= 1, (s, v3)
    # ops 0 and 1 answer as before; an unknown op kind is an error
    assert boda_hip.variant_name(1, [2, 32, 14, 14, 48, 3, 3, 1, 1, 1, 1])
    with pytest.raises(boda_hip.BodaHipError):
        boda_hip.variant_name(4, [1] * 11)


def test_bck_pack_size():
    for op in bck_ops()[0]:
        s = ops.bck_conv_shape(op)
        n = boda_hip.conv_bck_filts_packed_floats(s)
        t = ops.ConvShape(s.B, s.OC, s.OH, s.OW, s.IC, s.KY, s.KX, 1, 1, 0, 0)  # the transposed bank's forward op
        assert n >= s.OC * s.IC * s.KY * s.KX + boda_hip.conv_filts_packed_floats(t) > 0
        assert n % 4 == 0
