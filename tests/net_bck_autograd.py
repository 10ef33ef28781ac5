"""torch.autograd reference of a boda_hip_rtc_fwd --add-bck-ops run, as a program:

    net_bck_autograd.py PLAN.json BLOBDIR DROP_SEED

Builds the net of the plan JSON in float64 with the executor's synthetic parameters (oracle/net.py), its
input, its labels and the dropout mask of oracle/layers.py, runs loss.backward(), and compares the loss and
every *_grad_loss blob of BLOBDIR: rel-L2 <= 1e-4 and max|d| / max(1, max|ref|) <= 1e-3 (the per-blob bars
of tests/test_gpu_net.py). A blob's gradient buffer ends as the gradient of the value the blob had before
the in-place ops on it (ReLU, Dropout) ran, since their backward ops run in place too; a blob with several
consumers has one partial per consumer, in the order of the plan's Reduce op. Prints one line per blob and
exits 1 on a miss. It is a program of its own because torch brings a HIP runtime of its own, and a process
that has loaded it no longer finds the GPU through libboda_hip.so."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import layers as L  # noqa: E402
from oracle import net as N  # noqa: E402

F32 = np.float32
LABEL_SEED = 90417263


def labels(n, C):
    v = (N.det_hash_rand_vec(n, LABEL_SEED) + F32(5.0)) / F32(10.0) * F32(C)
    return np.minimum(F32(C - 1), np.floor(v)).astype(np.int64)


def main(plan_fn, blob_dir, drop_seed):
    plan = json.load(open(plan_fn))
    fwd = [o for o in plan["ops"] if not o.get("bck")]
    partials = {o["tops"][0][:-len("_grad_loss")]: list(o["bots"]) for o in plan["ops"] if o["type"] == "Reduce"}
    dt = torch.float64
    din, dlab = plan["inputs"][0], plan["inputs"][1]
    x = N.det_hash_rand_vec(int(np.prod(din["dims"])), N.IN_SEED).reshape(din["dims"])
    blobs = {din["name"]: torch.tensor(x, dtype=dt)}
    grads = {}  # gradient blob name -> the tensor whose .grad it is
    nreads = {}
    losses, C = [], None

    def read(name, in_place):
        t = blobs[name]
        if in_place or name not in partials:
            return t
        k = nreads.get(name, 0)
        nreads[name] = k + 1
        a = t * 1.0  # this consumer's own alias: its .grad is the consumer's partial
        a.retain_grad()
        grads[partials[name][k]] = a
        return a

    def write(name, t, first=None):
        first = t if first is None else first
        if name not in blobs and first.requires_grad:
            first.retain_grad()
            grads[name + "_grad_loss"] = first
        blobs[name] = t

    for op in fwd:
        t, tag = op["type"], op["tag"]
        in_place = op["tops"] == op["bots"]
        a = read(op["bots"][0], in_place)
        if t in ("Convolution", "InnerProduct"):
            Cin, H, W = a.shape[1:]
            ip = t == "InnerProduct"
            KY, KX = (H, W) if ip else op["k"]
            s, p = ((1, 1), (0, 0)) if ip else (op["s"], op["p"])
            OC = op["out_chans"]
            w = torch.tensor(N.synth(OC * Cin * KY * KX, tag, "filts", N.conv_scale(Cin * KY * KX)).reshape(OC, Cin, KY, KX),
                             dtype=dt, requires_grad=True)
            b = torch.tensor(N.synth(OC, tag, "biases", 0.1 / 5.0) if op["bias"] else np.zeros(OC, F32), dtype=dt,
                             requires_grad=True)
            grads[tag + "_filts_grad_loss"], grads[tag + "_biases_grad_loss"] = w, b
            pre = F.conv2d(a, w, b, stride=tuple(s), padding=tuple(p))
            write(op["tops"][0], F.relu(pre) if op["relu"] else pre, pre)
        elif t == "ReLU":
            write(op["tops"][0], F.relu(a))
        elif t == "Dropout":
            mask = L.dropout(np.ones(tuple(a.shape), F32), op["ratio"], drop_seed)
            write(op["tops"][0], a * torch.tensor(mask, dtype=dt))
        elif t == "Pooling":
            if op["global"]:
                out = a.mean((2, 3), keepdim=True) if op["avg"] else a.amax((2, 3), keepdim=True)
            else:
                f = F.avg_pool2d if op["avg"] else F.max_pool2d
                out = f(a, tuple(op["k"]), tuple(op["s"]), tuple(op["p"]), ceil_mode=True)
            write(op["tops"][0], out)
        elif t == "LRN":
            write(op["tops"][0], F.local_response_norm(a, op["local_size"], float(F32(op["alpha"])), float(F32(op["beta"])),
                                                       float(F32(op["kk"]))))
        elif t == "Concat":
            write(op["tops"][0], torch.cat([a] + [read(b, False) for b in op["bots"][1:]], 1))
        elif t == "SoftmaxWithLoss":
            B, C, H, W = a.shape
            lab = torch.tensor(labels(B * H * W, C).reshape(B, H, W))
            loss = F.cross_entropy(a, lab, reduction="none").mean(0)  # y x x, the mean over the batch
            losses.append(loss.sum())
            blobs[op["tops"][1]] = loss
            if a is not blobs[op["bots"][0]]:  # (a consumer's alias of a fan-out blob: the op's top is its partial)
                grads[op["tops"][0]] = a
        else:
            raise SystemExit("no torch restatement for layer type " + t)
        assert list(blobs[op["tops"][-1]].shape) == (op["out_dims"] if t != "SoftmaxWithLoss" else list(loss.shape)), tag
    sum(losses).backward()
    idx = {b["name"]: b for b in json.load(open(os.path.join(blob_dir, "blobs.json")))["blobs"]}
    ok, seen = True, 0
    for name, b in sorted(idx.items()):
        is_loss = any(name == o["tops"][1] for o in fwd if o["type"] == "SoftmaxWithLoss")
        if not (name.endswith("_grad_loss") or is_loss):
            continue
        got = np.fromfile(os.path.join(blob_dir, b["file"]), F32).astype(np.float64)
        if is_loss:
            ref = blobs[name].detach().numpy().reshape(-1)
        else:
            if name not in grads:
                print("MISS no reference for", name)
                ok = False
                continue
            ref = grads[name].grad.numpy().reshape(-1)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        rl2 = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
        nm = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
        good = rl2 <= 1e-4 and nm <= 1e-3 and np.abs(ref).max() > 0
        print("%s %-40s rel_l2=%.3e nmax=%.3e max|ref|=%.3e" % ("ok  " if good else "MISS", name, rl2, nm, np.abs(ref).max()))
        ok, seen = ok and good, seen + 1
    print("compared", seen)
    return 0 if ok and seen else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], int(sys.argv[3])))
