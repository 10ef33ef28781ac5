"""A whole net's gradient run: boda_hip_rtc_fwd --add-bck-ops --save-blobs on two tiny nets (net_bck_protos.py)
against torch.autograd on the CPU (net_bck_autograd.py, a process of its own): the loss and every *_grad_loss
blob at rel-L2 <= 1e-4 and normalised max <= 1e-3, and the forward blobs of the same run bit-identical to a run
without the flag. These are the tests of the backward ops composed as a net: ZeroIfNonPos before the fused
conv's BckConv, Reduce over the partials of a fan-out blob, Split's channel offsets, the first conv without an
input gradient."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

import net_bck_protos as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "boda-1_amd", "bin", "boda_hip_rtc_fwd")
SEED = 7


def run(args, timeout=120):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("name", ["CHAIN", "INCEPTION"])
def test_net_gradients_match_autograd(name, tmp_path):
    if importlib.util.find_spec("torch") is None:  # (looked up, not loaded into this process: see net_bck_autograd.py)
        pytest.skip("no torch")
    pt, plan_fn = tmp_path / "net.prototxt", tmp_path / "plan.json"
    bck, fwd = tmp_path / "bck", tmp_path / "fwd"
    pt.write_text(getattr(P, name))
    bck.mkdir()
    fwd.mkdir()
    plan = run(["--net", pt, "--add-bck-ops", "--plan-json"])
    plan_fn.write_text(plan)
    out = run(["--net", pt, "--add-bck-ops", "--det-dropout", SEED, "--iters", 1, "--save-blobs", bck])
    ops = json.loads(plan)["ops"]
    for o in ops:  # get_info_log lists the backward calls with their times
        if o.get("bck"):
            assert " " + o["tag"] + " " in out, (o["tag"], out)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "net_bck_autograd.py"), str(plan_fn), str(bck), str(SEED)],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout + r.stderr[-3000:])
    assert r.returncode == 0
    # every gradient blob of the plan was saved and compared
    want = {t for o in ops if o.get("bck") for t in o["tops"] if t} | {o["tops"][0] for o in ops if o["type"] == "SoftmaxWithLoss"}
    assert "compared %d\n" % (len(want) + 1) in r.stdout, sorted(want)
    # the forward blobs equal a run without the flag, bit for bit
    run(["--net", pt, "--det-dropout", SEED, "--iters", 1, "--no-inplace-concat", "--no-resadd", "--save-blobs", fwd])
    fidx = json.load(open(fwd / "blobs.json"))["blobs"]
    assert len(fidx) >= 5
    for b in fidx:
        assert (fwd / b["file"]).read_bytes() == (bck / b["file"]).read_bytes(), b["name"]


def test_net_gradients_under_graph(tmp_path):
    """--graph captures the forward and backward run as one graph and replays it."""
    pt = tmp_path / "net.prototxt"
    pt.write_text(P.INCEPTION)
    out = run(["--net", pt, "--add-bck-ops", "--iters", 1, "--graph", 3])
    n_calls = out.count("_bck ") + out.count("hip_conv__") + out.count("hip_pool__") + 1
    assert "as one hipGraph (" in out and n_calls > 10
