"""Planning of the backward pass, no GPU: boda_hip_rtc_fwd --add-bck-ops --plan-json on the reference nets.
One backward op per forward op (Pooling -> Spreading, ReLU -> ZeroIfNonPos, Dropout -> BckDropout,
LRN -> BckLRN, Concat -> Split, Convolution / InnerProduct -> BckConv), a Reduce per fan-out blob, every
*_grad_loss blob with the dims of its blob, BatchNorm refused by name, and nothing changed without the flag."""
import collections
import hashlib
import json
import os
import subprocess

import pytest

import net_bck_protos as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "boda-1_amd", "bin", "boda_hip_rtc_fwd")
NETS = os.path.join(ROOT, "tests", "golden", "nets")
BCK_OF = {"Pooling": "Spreading", "ReLU": "ZeroIfNonPos", "Dropout": "BckDropout", "LRN": "BckLRN", "Concat": "Split",
          "Convolution": "BckConv", "InnerProduct": "BckConv"}


def plan(net, *extra, raw=False):
    fn = net if os.path.isabs(str(net)) else os.path.join(NETS, net + ".prototxt")
    r = subprocess.run([BIN, "--net", str(fn), "--img", "2", "--plan-json"] + list(extra), capture_output=True, text=True)
    if raw:
        return r
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.mark.parametrize("net", ["alexnet_ng_conv", "nin_imagenet", "googlenet_conv"])
def test_one_backward_op_per_forward_op(net):
    p = plan(net, "--add-bck-ops")
    text = subprocess.run([BIN, "--net", os.path.join(NETS, net + ".prototxt"), "--img", "2", "--plan", "--add-bck-ops"],
                          capture_output=True, text=True).stdout
    fwd = [o for o in p["ops"] if not o.get("bck")]
    bck = [o for o in p["ops"] if o.get("bck")]
    assert p["ops"] == fwd + bck  # the backward ops come after the forward ones
    # --plan-json leaves fused ReLUs out of the forward list; --plan --add-bck-ops lists their ZeroIfNonPos
    want = collections.Counter(BCK_OF[o["type"]] for o in fwd if o["type"] != "SoftmaxWithLoss")
    want["ZeroIfNonPos"] += sum(o["relu"] for o in fwd)
    got = collections.Counter(o["type"] for o in bck)
    n_reduce = got.pop("Reduce", 0)
    assert got == want
    for o in bck:
        assert (o["type"] + " " + o["tag"] + " ") in text
    # a Reduce for every blob with several consumers, over one partial per consumer
    readers = collections.Counter(b for o in fwd if o["tops"] != o["bots"] for b in o["bots"])
    fan = {b for b, n in readers.items() if n > 1 and b != "label"}
    assert {o["tops"][0] for o in bck if o["type"] == "Reduce"} == {b + "_grad_loss" for b in fan} and n_reduce == len(fan)
    for o in bck:
        if o["type"] == "Reduce":
            assert len(o["bots"]) == readers[o["tops"][0][:-len("_grad_loss")]]
    if net == "googlenet_conv":
        assert got["Split"] == 9 and n_reduce == 9
    # dims: every gradient blob has its blob's dims; the first conv has no input gradient
    dims = {i["name"]: i["dims"] for i in p["inputs"]}
    for o in fwd:
        dims[o["tops"][0]] = o["out_dims"]
    assert dims["label"] == [2, 1, 1]
    blob_of = {b: o["tops"][0][:-len("_grad_loss")] for o in bck if o["type"] == "Reduce" for b in o["bots"]}  # partials
    seen = set()
    for o in bck:
        for t, d in zip(o["tops"], o["top_dims"]):
            seen.add(t)
            if o["type"] == "BckConv" and t != o["tops"][0]:  # <layer>_filts_grad_loss / <layer>_biases_grad_loss
                assert t.startswith(o["tag"][:-len("_bck")] + "_") and d[0] == dims[o["bots"][3][:-len("_grad_loss")]][1]
            elif t:
                assert t.endswith("_grad_loss") and d == dims[blob_of.get(t, t[:-len("_grad_loss")])], (t, d)
    assert "" in seen and "data_grad_loss" not in seen
    loss = [o for o in fwd if o["type"] == "SoftmaxWithLoss"]
    assert loss and all(o["tops"][0] == o["bots"][0] + "_grad_loss" and o["bots"][1] == "label" for o in loss)


def test_resnet_names_batchnorm():
    r = plan("resnet-50", "--add-bck-ops", raw=True)
    assert r.returncode != 0 and "BatchNorm" in r.stderr and "bn_conv1" in r.stderr


@pytest.mark.parametrize("net", ["alexnet_ng_conv", "nin_imagenet", "googlenet_conv", "resnet-50", "vgg_19"])
def test_plan_unchanged_without_the_flag(net):
    """Without --add-bck-ops the plan has no backward op, no label input and no key of the new ones; the
    forward ops of a plan with the flag differ only by what the TRAIN phase keeps (Dropout, the loss)."""
    # byte for byte what it was before the flag existed (sha256 of --img 2 --plan-json, recorded then)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "net_plan_json_sha256.json")))[net]
    assert hashlib.sha256(plan(net, raw=True).stdout.encode()).hexdigest() == want
    p = plan(net)
    assert [i["name"] for i in p["inputs"]] == ["data"]
    assert not any("bck" in o or "top_dims" in o or o["type"] == "SoftmaxWithLoss" for o in p["ops"])
    if net in ("resnet-50",):
        return
    q = plan(net, "--add-bck-ops")
    kept = [o for o in q["ops"] if not o.get("bck") and o["type"] not in ("Dropout", "SoftmaxWithLoss")]
    assert kept == p["ops"]


def test_tiny_nets_plan(tmp_path):
    for name, n_reduce in (("CHAIN", 0), ("INCEPTION", 1)):
        f = tmp_path / (name + ".prototxt")
        f.write_text(getattr(P, name))
        p = plan(f, "--add-bck-ops")
        bck = [o for o in p["ops"] if o.get("bck")]
        assert sum(o["type"] == "Reduce" for o in bck) == n_reduce
        assert bck[-1]["type"] == "BckConv" and bck[-1]["tops"][0] == ""
    split = [o for o in bck if o["type"] == "Split"][0]
    assert split["tops"] == ["b1_grad_loss", "b2_grad_loss", "b3_grad_loss"] and split["top_dims"][0] == [2, 4, 17, 17]


def test_net_top_without_loss_is_an_error(tmp_path):
    f = tmp_path / "n.prototxt"
    f.write_text(P.CHAIN.replace('layer { name: "loss"', 'layer { name: "acc" type: "Accuracy" bottom: "gpool" bottom: "label" }\n#'))
    r = plan(f, "--add-bck-ops", raw=True)
    assert r.returncode != 0 and "gpool" in r.stderr and "SoftmaxWithLoss" in r.stderr
