"""boda_hip_ops_prof over BckConv ops: the tuning-free route of each op against the ref64 known-good tune.

The op list is built from the 10 BckConv lines of op_sigs.txt. Those are signatures (kern_sz / stride /
in_pad, no tensor dims), so each stands for the op of op_sigs_full.txt with that signature and the least
work (ref64 runs one thread per output). The three gradients are generated-input outputs of one timed
call, digested and compared element-wise with the known-good tune at 2e-3, the project's live floor for
fp32 routes against the exact sum (tests/test_gpu_opsprof.py).
"""
import os
import re
import subprocess

import pytest

from boda_hip import ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "boda-1_amd", "bin", "boda_hip_ops_prof")
OPS = os.path.join(ROOT, "tests", "golden", "ops")


def sig_of(op):
    return tuple(tuple(op.dims[n].values()) for n in ("kern_sz", "stride", "in_pad"))


def bck_op_list():
    sigs, _ = ops.read_ops(os.path.join(OPS, "op_sigs.txt"), types=("BckConv",))
    full, _ = ops.read_ops(os.path.join(OPS, "op_sigs_full.txt"), types=("BckConv",))
    assert len(sigs) == 10
    out = []
    for sg in sigs:
        cands = [o for o in full if sig_of(o) == sig_of(sg)]
        assert cands, sg.line
        out.append(min(cands, key=lambda o: ops.bck_flops(ops.bck_conv_shape(o))))
    return out


def test_ops_prof_bck_vs_ref64(tmp_path):
    lst = bck_op_list()
    ops_fn, wout = tmp_path / "ops.txt", tmp_path / "out.wis"
    ops_fn.write_text("".join(o.line + "\n" for o in lst))
    r = subprocess.run([BIN, "--ops-fn=" + str(ops_fn), "--op-tunes=(kg=(use_be=hip,cfg=ref64),tab=(use_be=hip))",
                        "--kg-tune-tag=kg", "--gen-data-mode=5", "--live-mrd-toler=2e-3", "--write-runs=1",
                        "--wisdom-out-fn=" + str(wout)], capture_output=True, text=True, timeout=110)
    print(r.stdout[-4000:])
    runs = re.findall(r"op_ix=(\d+) tune=(\S+) func=(\S+) .* mrd_vs_kg=(\S+) toler=(\S+) comp=(\w+)", r.stdout)
    assert len([x for x in runs if x[1] == "kg"]) == 10 and len([x for x in runs if x[1] == "tab"]) == 10
    assert all(x[2] == "ref64_bck_in_double+ref64_bck_filts_double" for x in runs if x[1] == "kg"), runs
    assert all(x[2].startswith(("bck_in_fwd:", "mfma32_bcki_")) and "+mfma32_bckf_" in x[2] for x in runs if x[1] == "tab")
    assert not [x for x in runs if x[5] != "ok"], [x for x in runs if x[5] != "ok"]
    assert r.returncode == 0 and "***ALL IS WELL***" in r.stdout, r.stdout[-4000:] + r.stderr
    assert "unsupported" not in r.stdout
    st = subprocess.run([BIN, "--selftest-wisdom=" + str(wout)], capture_output=True, text=True, timeout=60)
    assert st.returncode == 0, st.stdout + st.stderr
