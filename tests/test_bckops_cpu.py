"""CPU-only checks of the backward ops of the non-conv layers (no GPU):

* the float64 restatements of tests/bckops_ref.py agree with torch.autograd where the two definitions
  coincide: whole-window pooling without ties, LRN, cross-entropy with mean over the batch -- and with
  hand-computed answers where they do not (truncated average windows);
* libboda_hip.so exports the new entries and boda_hip.EXPORTS lists them;
* the Python and C++ op-list readers agree on every backward op of op_sigs_full.txt under the work
  model of DESIGN.md 8c, and both reject an inconsistent line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import bckops_ref as R
import boda_hip
from boda_hip import ops
from oracle import layers as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = os.path.join(ROOT, "tests", "golden", "ops")
BIN = os.path.join(ROOT, "boda-1_amd", "bin", "boda_hip_ops_prof")
NEW = ["bh_spreading_nchw", "bh_lrn_bck_nchw", "bh_zero_if_non_pos", "bh_reduce_sum", "bh_sm_grad_and_loss",
       "bh_sum_loss_over_imgs", "bh_softmax_with_loss"]
BCK_TYPES = {"Spreading": 23, "BckLRN": 4, "ZeroIfNonPos": 58, "BckDropout": 5, "Reduce": 13, "SoftmaxWithLoss": 3}


def _rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


# ---- restatements against torch.autograd
def test_restatements_match_autograd():
    """bckops_autograd_check.py in a process of its own (it says why): Spreading at 5 shapes, BckLRN at 3,
    the loss gradient at 2."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bckops_autograd_check.py")], capture_output=True,
                       text=True, timeout=120)
    if r.returncode == 3:
        pytest.skip("no torch")
    assert r.returncode == 0 and r.stdout.count("ok ") == 10, r.stdout + r.stderr


def test_spreading_restatement_truncated_average():
    # 1 x 1 x 3 x 3, 2x2 stride 2: windows of 4, 2, 2 and 1 in-image taps; each divides by its own count
    og = np.array([[[[4.0, 2.0], [6.0, 5.0]]]], np.float32)
    ref, aref, cnt = R.spreading(og, None, (1, 1, 3, 3), 2, 2, 2, 2, 0, 0, 1)
    np.testing.assert_array_equal(ref[0, 0], [[1, 1, 1], [1, 1, 1], [3, 3, 5]])
    np.testing.assert_array_equal(cnt[0, 0], np.ones((3, 3)))
    np.testing.assert_array_equal(aref, np.abs(ref))


def test_spreading_restatement_ties_and_no_winner():
    og = np.array([[[[1.0, 2.0]]]], np.float32)  # 1 x 3 input, k2 s1: both windows point at pixel 1
    ref, _, cnt = R.spreading(og, np.array([[[[1.0, 1.0]]]], np.float32), (1, 1, 1, 3), 1, 2, 1, 1, 0, 0, 0)
    np.testing.assert_array_equal(ref[0, 0], [[0, 3, 0]])
    np.testing.assert_array_equal(cnt[0, 0], [[1, 2, 1]])
    ref, _, _ = R.spreading(og, np.array([[[[-1.0, -1.0]]]], np.float32), (1, 1, 1, 3), 1, 2, 1, 1, 0, 0, 0)
    assert (ref == 0).all()


def test_elementwise_restatements():
    x = np.array([1.0, np.nan, 3.0, np.nan, 5.0], np.float32)
    cond = np.array([0.0, -0.0, np.nan, 1.0, 2.0], np.float32)
    got = R.zero_if_non_pos(x, cond)
    np.testing.assert_array_equal(got[:3], [0, 0, 0])
    assert np.isnan(got[3]) and got[4] == 5
    big = [np.array([1e8], np.float32), np.array([1.0], np.float32), np.array([-1e8], np.float32)]
    assert R.reduce_sum_f32(big)[0] == 0.0 and R.reduce_sum_f32(big[::-1])[0] == 0.0
    assert R.reduce_sum_f32([big[0], big[2], big[1]])[0] == 1.0  # the order is the definition


# ---- the library
def test_library_exports_backward_ops():
    lib = ctypes.CDLL(boda_hip.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in boda_hip.EXPORTS
    assert boda_hip.lib().bh_abi_version() == 3
    for name in ("spreading", "lrn_bck", "zero_if_non_pos", "reduce_sum", "sm_grad_and_loss", "sum_loss_over_imgs",
                 "softmax_with_loss"):
        assert callable(getattr(boda_hip.Device, name))


# ---- the op-list readers and the work model
def _dump(path, types):
    return subprocess.run([BIN, "--dump-ops=" + path, "--types=" + ",".join(types)], capture_output=True, text=True)


def test_cpp_and_python_parse_agree_on_backward_ops():
    fn = os.path.join(OPS, "op_sigs_full.txt")
    r = _dump(fn, list(BCK_TYPES))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    py, skipped = ops.read_ops(fn, types=tuple(BCK_TYPES))
    assert lines[-1] == "skipped %d" % skipped
    assert len(lines) - 1 == len(py) == sum(BCK_TYPES.values())
    count = dict.fromkeys(BCK_TYPES, 0)
    for l, op in zip(lines, py):
        f = l.split()
        s = ops.shape_of(op)
        count[op.type] += 1
        assert f[0] == op.type and [int(x) for x in f[1:-2]] == s.as_dims()
        assert (int(f[-2]), int(f[-1])) == (s.flops(), s.bytes())
    assert count == BCK_TYPES


def test_read_ops_defaults_unchanged():
    py, skipped = ops.read_ops(os.path.join(OPS, "op_sigs_full.txt"))
    assert {op.type for op in py} <= {"Convolution", "sgemm"} and skipped >= sum(BCK_TYPES.values())


def test_work_model_by_hand():
    def shape(line):
        return ops.shape_of(ops.parse_op(line))
    t = "(img=2,chan=3,y=5,x=7)"
    s = shape("(type=ZeroIfNonPos,dims_vals=(cond=%s,in=%s,out=%s))" % (t, t, t))
    assert (s.flops(), s.bytes()) == (0, 4 * 3 * 210)
    s = shape("(type=BckDropout,dims_vals=(in=%s,out=%s),str_vals=(dropout_ratio=0.5))" % (t, t))
    assert (s.flops(), s.bytes()) == (210, 4 * 2 * 210)
    s = shape("(type=Reduce,dims_vals=(ins_0=%s,ins_1=%s,ins_2=%s,out=%s))" % (t, t, t, t))
    assert (s.n_ins, s.flops(), s.bytes()) == (3, 3 * 210, 4 * 4 * 210)
    s = shape("(type=BckLRN,dims_vals=(in=%s,in_grad_loss=%s,out=%s,out_grad_loss=%s),"
              "str_vals=(alpha=0.0001,beta=0.75,k=1,local_size=5))" % (t, t, t, t))
    assert (s.flops(), s.bytes()) == (210 * 13, 4 * 5 * 210)
    s = shape("(type=SoftmaxWithLoss,dims_vals=(in=%s,in_grad_loss=%s,label=(img=2,y=5,x=7),loss=(y=5,x=7)))" % (t, t))
    assert (s.flops(), s.bytes()) == (3 * 210, 4 * (3 * 210 + 2 * 70 + 35))
    t, o = "(img=2,chan=3,y=6,x=8)", "(img=2,chan=3,y=3,x=4)"  # 3x3 stride 2 over 6 x 8, the ceil rule: 3 x 4
    s = shape("(type=Spreading,dims_vals=(in=%s,in_grad_loss=%s,in_pad=(y=0,x=0),kern_sz=(y=3,x=3),out=%s,"
              "out_grad_loss=%s,stride=(y=2,x=2)),str_vals=(avg_pool=0,emit_out_in_yx=1))" % (t, t, o, o))
    assert (s.OH, s.OW, s.flops(), s.bytes()) == (3, 4, 288 * 4, 4 * (2 * 72 + 288))


def test_spreading_without_kern_sz_is_global():
    fn = os.path.join(OPS, "op_sigs_full.txt")
    py, _ = ops.read_ops(fn, types=("Spreading",))
    bare = [op for op in py if "kern_sz" not in op.dims]
    assert len(bare) == 1
    s = ops.shape_of(bare[0])
    assert (s.KY, s.KX, s.OH, s.OW, s.avg) == (s.H, s.W, 1, 1, 1)
    assert s.bytes() == 4 * (s.B * s.C + s.N)


BAD = [  # each with one tensor a row short (or a tensor missing)
    "(type=ZeroIfNonPos,dims_vals=(cond=(img=1,chan=4,y=5,x=6),in=(img=1,chan=4,y=6,x=6),out=(img=1,chan=4,y=6,x=6)))",
    "(type=BckDropout,dims_vals=(in=(img=1,chan=4,y=6,x=6),out=(img=1,chan=4,y=5,x=6)),str_vals=(dropout_ratio=0.5))",
    "(type=Reduce,dims_vals=(ins_0=(img=1,chan=4,y=6,x=6),ins_1=(img=1,chan=4,y=5,x=6),out=(img=1,chan=4,y=6,x=6)))",
    "(type=Reduce,dims_vals=(ins_0=(img=1,chan=4,y=6,x=6),ins_2=(img=1,chan=4,y=6,x=6),out=(img=1,chan=4,y=6,x=6)))",
    "(type=BckLRN,dims_vals=(in=(img=1,chan=4,y=6,x=6),in_grad_loss=(img=1,chan=4,y=6,x=6),out=(img=1,chan=4,y=6,x=6),"
    "out_grad_loss=(img=1,chan=4,y=5,x=6)),str_vals=(alpha=0.0001,beta=0.75,k=1,local_size=5))",
    "(type=SoftmaxWithLoss,dims_vals=(in=(img=2,chan=9,y=2,x=1),in_grad_loss=(img=2,chan=9,y=2,x=1),"
    "label=(img=2,y=1,x=1),loss=(y=2,x=1)))",
    "(type=Spreading,dims_vals=(in=(img=1,chan=4,y=13,x=13),in_grad_loss=(img=1,chan=4,y=13,x=13),in_pad=(y=0,x=0),"
    "kern_sz=(y=3,x=3),out=(img=1,chan=4,y=6,x=6),out_grad_loss=(img=1,chan=4,y=5,x=6),stride=(y=2,x=2)),"
    "str_vals=(avg_pool=0,emit_out_in_yx=1))",
    "(type=Spreading,dims_vals=(in=(img=1,chan=4,y=13,x=13),in_grad_loss=(img=1,chan=4,y=12,x=13),in_pad=(y=0,x=0),"
    "out=(img=1,chan=4,y=1,x=1),out_grad_loss=(img=1,chan=4,y=1,x=1),stride=(y=1,x=1)),str_vals=(avg_pool=1))",
]


@pytest.mark.parametrize("line", BAD, ids=lambda l: l[6:l.index(",")] + str(abs(hash(l)) % 97))
def test_inconsistent_line_raises_in_both_readers(line, tmp_path):
    op = ops.parse_op(line)
    with pytest.raises(ValueError):
        ops.shape_of(op)
    fn = tmp_path / "ops.txt"
    fn.write_text(line + "\n")
    r = _dump(str(fn), [op.type])
    assert r.returncode != 0 and "skipped" not in r.stdout
