"""boda_hip_ops_prof over the backward ops of the non-conv layers: the production kernel of each op against
its ref64 known-good tune, through hip_compute_t's function kinds (hip_spreading, hip_bck_lrn,
hip_zero_if_non_pos, hip_reduce, hip_softmax_with_loss; BckDropout on hip_dropout, Split on hip_copy).

One op per type: the line of op_sigs_full.txt with the least work (bytes of the work model).
Inputs are generated on the device; out / out_in_yx and out / out_scale_base come from an untimed forward
call. Each type is compared element-wise with the known-good tune at its own bar:

* Spreading: T * 2^-23, T the windows that can cover a pixel (fp32 summation of T terms);
* BckLRN: 4e-6 (the bar of tests/test_gpu_bckops.py);
* Reduce: n_ins * 2^-23 (fp32 left-to-right sum against the double sum rounded once);
* SoftmaxWithLoss: 1e-6, the gradient's bar, which is the tighter of its two;
* ZeroIfNonPos, BckDropout, Split: no arithmetic that rounds differently, so any difference fails.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import boda_hip
from boda_hip import ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "boda-1_amd", "bin", "boda_hip_ops_prof")
FULL = os.path.join(ROOT, "tests", "golden", "ops", "op_sigs_full.txt")
EXACT = 1e-30  # ops-prof fails a compare at mrd >= toler: with this, any non-zero difference
NAME = {"Spreading": "spreading", "BckLRN": "bck_lrn", "ZeroIfNonPos": "zero_if_non_pos", "BckDropout": "dropout",
        "Reduce": "reduce", "SoftmaxWithLoss": "softmax_with_loss"}


def least_work(t):
    lst, _ = ops.read_ops(FULL, types=(t,))
    return min(lst, key=lambda o: ops.shape_of(o).bytes())


def bar_of(op):
    s = ops.shape_of(op)
    return {"Spreading": lambda: -(-s.KY // s.sy) * -(-s.KX // s.sx) * 2.0 ** -23, "BckLRN": lambda: 4e-6,
            "Reduce": lambda: s.n_ins * 2.0 ** -23, "SoftmaxWithLoss": lambda: 1e-6}.get(op.type, lambda: EXACT)()


def run_prof(tmp_path, line, tunes, toler):
    ops_fn, wout = tmp_path / "ops.txt", tmp_path / "out.wis"
    ops_fn.write_text(line + "\n")
    r = subprocess.run([BIN, "--ops-fn=" + str(ops_fn), "--op-tunes=" + tunes, "--kg-tune-tag=kg", "--gen-data-mode=5",
                        "--mrd-toler=%g" % toler, "--live-mrd-toler=%g" % toler, "--write-runs=1",
                        "--wisdom-out-fn=" + str(wout)], capture_output=True, text=True, timeout=60)
    print(r.stdout[-3000:] + r.stderr[-1000:])
    return r, wout


@pytest.mark.parametrize("t", sorted(NAME))
def test_ops_prof_bck_op_vs_ref64(t, tmp_path):
    op = least_work(t)
    r, wout = run_prof(tmp_path, op.line, "(kg=(use_be=hip,cfg=ref64),tab=(use_be=hip))", bar_of(op))
    runs = dict(re.findall(r"tune=(\S+) func=(\S+) ", r.stdout))
    assert runs == {"kg": "ref64_" + NAME[t], "tab": "bckop_" + NAME[t]}, r.stdout
    assert re.findall(r"comp=(\w+)", r.stdout) == ["ok", "ok"]
    assert r.returncode == 0 and "***ALL IS WELL***" in r.stdout and "unsupported" not in r.stdout
    st = subprocess.run([BIN, "--selftest-wisdom=" + str(wout)], capture_output=True, text=True, timeout=60)
    assert st.returncode == 0 and "selftest ok: " in st.stdout, st.stdout + st.stderr


def test_ops_prof_split_is_chan_copies(tmp_path):
    lst, _ = ops.read_ops(FULL, types=("Split",))
    op = min(lst, key=lambda o: len(o.line))
    r, _ = run_prof(tmp_path, op.line, "(kg=(use_be=hip))", EXACT)
    assert r.returncode == 0 and "***ALL IS WELL***" in r.stdout and "unsupported" not in r.stdout
    assert "func=hip_copy " in r.stdout


def test_ops_prof_bck_op_other_cfg_is_unsupported(tmp_path):
    r, _ = run_prof(tmp_path, least_work("ZeroIfNonPos").line, "(kg=(use_be=hip,cfg=ref64),bad=(use_be=hip,cfg=mfma32))", EXACT)
    assert "no ZeroIfNonPos configuration named 'mfma32'" in r.stdout
    assert "unsupported (recorded in wisdom, skipped): 1" in r.stdout


def test_gen_label_and_cond(dev):
    """BH_GEN_LABEL: hashed integers in [0, C) over img x y x x, C passed as d[3]; BH_GEN_COND: the
    Convolution in generator's modes with a seed of its own."""
    B, H, W, C = 5, 4, 7, 10
    lab = dev.alloc_floats(B * H * W + 3)
    lab.upload(np.full(B * H * W + 3, -7.0, np.float32))
    dev.gen_data(boda_hip.GEN_LABEL, lab, [B, H, W, C], 5)
    x = lab.download()
    assert (x[B * H * W:] == -7.0).all()  # writes img x y x x elements, not d[3] times as many
    x = x[:B * H * W]
    assert (x == np.floor(x)).all() and (x >= 0).all() and (x < C).all() and len(np.unique(x)) == C
    d = [2, 3, 5, 7]
    a, b = dev.alloc_floats(210), dev.alloc_floats(210)
    dev.gen_data(boda_hip.GEN_COND, a, d, 5)
    dev.gen_data(boda_hip.GEN_CONV_IN, b, d, 5)
    u, v = a.download(), b.download()
    assert (u >= -5).all() and (u < 5).all() and (u > 0).sum() > 50 and (u <= 0).sum() > 50 and (u != v).sum() > 200
    for t in (lab, a, b):
        t.free()
