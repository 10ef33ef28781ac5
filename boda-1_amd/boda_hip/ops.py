"""Boda op-line parsing and per-op work model (host-side glue).

Op lines come in two dialects:
  current  (str_vals=(type=Convolution),nda_vals=(in=(dims=(img=5,...)),
            kern_sz=(tn=none,dims=(y=3,x=3)),out_chans=(tn=uint32_t,v=256),...))
           -- op_base_t{str_vals,nda_vals}, src/op_base.H:9-14
  legacy   (type=Convolution,dims_vals=(in=(img=5,...),...),str_vals=(out_chans=256))
           -- emitted by pysrc/to-prof-ops-gen.py:66-68
Both are parsed with the lexp grammar of src/lexp.cc:253-330:
  lexp := '(' [name '=' lexp {',' name '=' lexp}] ')' | leaf
(a leaf runs to the next unbalanced ')' or ','; backslash escapes).

Flop / byte model: src/latex-util.H:101-136 (conv: M = B*OY*OX, K = IC*KY*KX,
N = OC, flops = 2MNK, bytes = 4*(in + out + filts + biases); sgemm: flops = 2MNK,
bytes = 4*(MK + KN + MN)).
"""
from collections import OrderedDict
from dataclasses import dataclass, field


class LexpError(ValueError):
    pass


def parse_lexp(s):
    """Parse one lexp string into nested OrderedDicts (leaves are str)."""
    pos = 0

    def leaf():
        nonlocal pos
        out, depth = [], 0
        while pos < len(s):
            ch = s[pos]
            if ch == "\\" and pos + 1 < len(s):
                out.append(s[pos + 1])
                pos += 2
                continue
            if ch == "(":
                depth += 1
            elif ch == ")":
                if depth == 0:
                    break
                depth -= 1
            elif ch == "," and depth == 0:
                break
            out.append(ch)
            pos += 1
        return "".join(out)

    def node():
        nonlocal pos
        if pos < len(s) and s[pos] == "(":
            pos += 1
            d = OrderedDict()
            if pos < len(s) and s[pos] == ")":
                pos += 1
                return d
            while True:
                eq = s.find("=", pos)
                if eq < 0:
                    raise LexpError("expected name= at %d in %r" % (pos, s))
                name = s[pos:eq]
                if not name or any(c in name for c in "(),"):
                    raise LexpError("bad name %r at %d" % (name, pos))
                pos = eq + 1
                if name in d:
                    raise LexpError("duplicate key %r" % name)
                d[name] = node()
                if pos >= len(s):
                    raise LexpError("unterminated list in %r" % s)
                if s[pos] == ",":
                    pos += 1
                    continue
                if s[pos] == ")":
                    pos += 1
                    return d
                raise LexpError("unexpected %r at %d" % (s[pos], pos))
        return leaf()

    v = node()
    if pos != len(s):
        raise LexpError("trailing text %r" % s[pos:])
    return v


@dataclass
class Op:
    type: str
    dims: "OrderedDict[str, OrderedDict[str, int]]" = field(default_factory=OrderedDict)
    scalars: "OrderedDict[str, int]" = field(default_factory=OrderedDict)
    strs: "OrderedDict[str, str]" = field(default_factory=OrderedDict)
    line: str = ""


def _dims(d):
    out = OrderedDict()
    for k, v in d.items():
        if k == "__tn__":
            continue
        out[k] = int(v)
    return out


def parse_op(line):
    """One op line (either dialect) -> Op."""
    line = line.strip()
    t = parse_lexp(line)
    if not isinstance(t, dict):
        raise LexpError("op line is not a list: %r" % line)
    if "nda_vals" in t or ("str_vals" in t and "type" in t.get("str_vals", {})):
        sv = t.get("str_vals", OrderedDict())
        op = Op(type=sv["type"], line=line)
        for k, v in sv.items():
            if k != "type":
                op.strs[k] = v
        for name, nda in t.get("nda_vals", OrderedDict()).items():
            if "dims" in nda:
                op.dims[name] = _dims(nda["dims"])
            elif "v" in nda:
                op.scalars[name] = int(nda["v"])
        return op
    if "type" in t:  # legacy dialect
        op = Op(type=t["type"], line=line)
        for name, dd in t.get("dims_vals", OrderedDict()).items():
            op.dims[name] = _dims(dd)
        for k, v in t.get("str_vals", OrderedDict()).items():
            try:
                op.scalars[k] = int(v)
            except ValueError:
                op.strs[k] = v
        return op
    raise LexpError("unrecognised op line: %r" % line)


def conv_out_sz(i, pad, k, stride):
    """src/conv_util.cc:167-173"""
    p = i + 2 * pad
    return 0 if p < k else (p - k) // stride + 1


@dataclass(frozen=True)
class ConvShape:
    B: int
    IC: int
    H: int
    W: int
    OC: int
    KY: int
    KX: int
    sy: int
    sx: int
    py: int
    px: int

    @property
    def OH(self):
        return conv_out_sz(self.H, self.py, self.KY, self.sy)

    @property
    def OW(self):
        return conv_out_sz(self.W, self.px, self.KX, self.sx)

    @property
    def M(self):
        return self.B * self.OH * self.OW

    @property
    def K(self):
        return self.IC * self.KY * self.KX

    @property
    def N(self):
        return self.OC

    def flops(self):
        return 2 * self.M * self.N * self.K

    def bytes(self):
        return 4 * (self.B * self.IC * self.H * self.W + self.B * self.OC * self.OH * self.OW
                    + self.OC * self.K + self.OC)

    def as_dims(self):
        return [self.B, self.IC, self.H, self.W, self.OC, self.KY, self.KX, self.sy, self.sx, self.py, self.px]


@dataclass(frozen=True)
class SgemmShape:
    M: int
    N: int
    K: int

    def flops(self):
        return 2 * self.M * self.N * self.K

    def bytes(self):
        return 4 * (self.M * self.K + self.K * self.N + self.M * self.N)


def conv_shape(op):
    """Op (type Convolution) -> ConvShape, checking the reference's consistency rules."""
    if op.type != "Convolution":
        raise ValueError("not a Convolution op: %s" % op.type)
    din, df = op.dims["in"], op.dims["filts"]
    ks, st, pd = op.dims["kern_sz"], op.dims["stride"], op.dims["in_pad"]
    s = ConvShape(B=din["img"], IC=din["chan"], H=din["y"], W=din["x"], OC=df["out_chan"],
                  KY=ks["y"], KX=ks["x"], sy=st["y"], sx=st["x"], py=pd["y"], px=pd["x"])
    if df["in_chan"] != s.IC or df["y"] != s.KY or df["x"] != s.KX:
        raise ValueError("filts dims inconsistent with in / kern_sz: %s" % op.line)
    if "out" in op.dims:
        do = op.dims["out"]
        if (do["img"], do["chan"], do["y"], do["x"]) != (s.B, s.OC, s.OH, s.OW):
            raise ValueError("out dims inconsistent with conv_in_sz_to_out_sz: %s" % op.line)
    oc = op.scalars.get("out_chans")
    if oc is not None and oc != s.OC:
        raise ValueError("out_chans mismatch: %s" % op.line)
    return s


def bck_conv_shape(op):
    """Op (type BckConv, src/conv_util.cc:65) -> the ConvShape of its forward op, checking that
    in_grad_loss / filts_grad_loss / biases_grad_loss have the dims of in / filts / biases and that
    out_grad_loss is B x OC x OH x OW of conv_in_sz_to_out_sz."""
    if op.type != "BckConv":
        raise ValueError("not a BckConv op: %s" % op.type)
    for n in ("in", "filts", "biases", "out_grad_loss", "kern_sz", "stride", "in_pad"):
        if n not in op.dims:
            raise ValueError("BckConv op without %s dims: %s" % (n, op.line))
    din, df = op.dims["in"], op.dims["filts"]
    ks, st, pd = op.dims["kern_sz"], op.dims["stride"], op.dims["in_pad"]
    s = ConvShape(B=din["img"], IC=din["chan"], H=din["y"], W=din["x"], OC=df["out_chan"],
                  KY=ks["y"], KX=ks["x"], sy=st["y"], sx=st["x"], py=pd["y"], px=pd["x"])
    if df["in_chan"] != s.IC or df["y"] != s.KY or df["x"] != s.KX:
        raise ValueError("filts dims inconsistent with in / kern_sz: %s" % op.line)
    if list(op.dims["biases"].values()) != [s.OC]:
        raise ValueError("biases dims inconsistent with filts: %s" % op.line)
    for g, v in (("in_grad_loss", "in"), ("filts_grad_loss", "filts"), ("biases_grad_loss", "biases")):
        if g in op.dims and list(op.dims[g].items()) != list(op.dims[v].items()):
            raise ValueError("%s dims differ from %s: %s" % (g, v, op.line))
    do = op.dims["out_grad_loss"]
    if (do["img"], do["chan"], do["y"], do["x"]) != (s.B, s.OC, s.OH, s.OW):
        raise ValueError("out_grad_loss dims inconsistent with conv_in_sz_to_out_sz: %s" % op.line)
    return s


def bck_flops(s):
    """BckConv work model (the reference gives none, src/cnn_op.cc:330): the input and the filter
    gradient each do the forward's M*N*K multiply-adds, the bias gradient M*N adds."""
    return 4 * s.M * s.N * s.K + s.M * s.N


def bck_bytes(s):
    """in and filts read, in_grad and filts_grad written, out_grad read, biases_grad written."""
    return 4 * (2 * s.B * s.IC * s.H * s.W + 2 * s.OC * s.K + s.B * s.OC * s.OH * s.OW + s.OC)


def pool_out_sz(i, pad, k, stride):
    """Caffe pooling: a partial last window adds an output (src/conv_util.cc:198-204)."""
    p = i + 2 * pad
    return 1 if p < k else -(-(p - k) // stride) + 1


@dataclass(frozen=True)
class BckOpShape:
    """One backward op of a non-conv layer (bh_bckops.hip): the B x C x H x W tensor its gradient has, and
    what its type adds: the pooling window (Spreading), local_size (BckLRN), n_ins (Reduce). The work
    model (op_desc.cc op_work states the same): bytes = 4 x the elements of every tensor
    the definition reads or writes."""
    type: str
    B: int
    C: int
    H: int
    W: int
    KY: int = 0
    KX: int = 0
    sy: int = 0
    sx: int = 0
    py: int = 0
    px: int = 0
    avg: int = 0
    local_size: int = 0
    n_ins: int = 0

    @property
    def N(self):
        return self.B * self.C * self.H * self.W

    @property
    def OH(self):
        return pool_out_sz(self.H, self.py, self.KY, self.sy)

    @property
    def OW(self):
        return pool_out_sz(self.W, self.px, self.KX, self.sx)

    def flops(self):
        t = self.type
        if t == "Spreading":  # the windows that can cover a pixel
            return self.N * -(-self.KY // self.sy) * -(-self.KX // self.sx)
        return {"ZeroIfNonPos": 0, "BckDropout": self.N, "Reduce": self.n_ins * self.N,
                "BckLRN": self.N * (self.local_size + 8), "SoftmaxWithLoss": 3 * self.N}[t]

    def bytes(self):
        t, n = self.type, self.N
        if t == "Spreading":  # out_grad_loss (+ out_in_yx for max) read, in_grad_loss written
            return 4 * ((1 if self.avg else 2) * self.B * self.C * self.OH * self.OW + n)
        if t == "SoftmaxWithLoss":  # in, prob, in_grad_loss; label, loss_per_pel; loss
            return 4 * (3 * n + 2 * self.B * self.H * self.W + self.H * self.W)
        # BckLRN: in, out, out_scale_base, out_grad_loss, in_grad_loss; BckDropout is in place
        return 4 * n * {"ZeroIfNonPos": 3, "BckDropout": 2, "Reduce": self.n_ins + 1, "BckLRN": 5}[t]

    def as_dims(self):
        d = [self.B, self.C, self.H, self.W]
        if self.type == "Spreading":
            d += [self.KY, self.KX, self.sy, self.sx, self.py, self.px, self.avg]
        elif self.type == "BckLRN":
            d += [self.local_size]
        elif self.type == "Reduce":
            d += [self.n_ins]
        return d


def _nchw(op, name):
    if name not in op.dims:
        raise ValueError("%s op without %s dims: %s" % (op.type, name, op.line))
    d = op.dims[name]
    if list(d.keys()) != ["img", "chan", "y", "x"]:
        raise ValueError("%s is not img x chan x y x x: %s" % (name, op.line))
    return (d["img"], d["chan"], d["y"], d["x"])


def _same(op, names, want):
    for n in names:
        if _nchw(op, n) != want:
            raise ValueError("%s dims differ from %s: %s" % (n, "x".join(map(str, want)), op.line))


def spreading_shape(op):
    """Op (type Spreading, src/conv_util.cc:40-64) -> BckOpShape: in_grad_loss has the dims of in, out (if
    listed) and out_grad_loss are B x C x OH x OW of the pooling size rule; a line without kern_sz
    pools globally (src/cnn_op.cc:42: the window is in's y x x)."""
    if op.type != "Spreading":
        raise ValueError("not a Spreading op: %s" % op.type)
    B, C, H, W = _nchw(op, "in")
    for n in ("stride", "in_pad"):
        if n not in op.dims:
            raise ValueError("Spreading op without %s dims: %s" % (n, op.line))
    ks = op.dims.get("kern_sz", {"y": H, "x": W})
    st, pd = op.dims["stride"], op.dims["in_pad"]
    s = BckOpShape("Spreading", B, C, H, W, KY=ks["y"], KX=ks["x"], sy=st["y"], sx=st["x"], py=pd["y"], px=pd["x"],
                   avg=int(op.scalars.get("avg_pool", 0)))
    if not (s.KY and s.KX and s.sy and s.sx):
        raise ValueError("zero kern_sz or stride: %s" % op.line)
    _same(op, ["in_grad_loss"], (B, C, H, W))
    _same(op, ["out_grad_loss"] + (["out"] if "out" in op.dims else []), (B, C, s.OH, s.OW))
    return s


def bck_lrn_shape(op):
    """Op (type BckLRN) -> BckOpShape: in, out, out_grad_loss and in_grad_loss have the same dims."""
    if op.type != "BckLRN":
        raise ValueError("not a BckLRN op: %s" % op.type)
    d = _nchw(op, "in")
    _same(op, ["out", "out_grad_loss", "in_grad_loss"], d)
    if "local_size" not in op.scalars:
        raise ValueError("BckLRN op without local_size: %s" % op.line)
    return BckOpShape("BckLRN", *d, local_size=int(op.scalars["local_size"]))


def softmax_loss_shape(op):
    """Op (type SoftmaxWithLoss) -> BckOpShape: in_grad_loss as in, label img x y x x, loss y x x."""
    if op.type != "SoftmaxWithLoss":
        raise ValueError("not a SoftmaxWithLoss op: %s" % op.type)
    B, C, H, W = d = _nchw(op, "in")
    _same(op, ["in_grad_loss"], d)
    for n, want in (("label", [("img", B), ("y", H), ("x", W)]), ("loss", [("y", H), ("x", W)])):
        if n not in op.dims or list(op.dims[n].items()) != want:
            raise ValueError("%s dims inconsistent with in: %s" % (n, op.line))
    return BckOpShape("SoftmaxWithLoss", *d)


ELEMENTWISE = {"ZeroIfNonPos": ("in", "cond", "out"), "BckDropout": ("in", "out"), "Reduce": ("out",)}


def elementwise_shape(op):
    """Op (type ZeroIfNonPos / BckDropout / Reduce) -> BckOpShape: every tensor has the same dims; Reduce
    lists ins_0 .. ins_{n-1}."""
    if op.type not in ELEMENTWISE:
        raise ValueError("not an elementwise backward op: %s" % op.type)
    names = list(ELEMENTWISE[op.type])
    n_ins = 0
    if op.type == "Reduce":
        while "ins_%d" % n_ins in op.dims:
            n_ins += 1
        if not n_ins or len(op.dims) != n_ins + 1:
            raise ValueError("Reduce op needs ins_0 .. ins_n-1 and out: %s" % op.line)
        names += ["ins_%d" % i for i in range(n_ins)]
    elif sorted(op.dims) != sorted(names):
        raise ValueError("%s op needs exactly %s: %s" % (op.type, ", ".join(names), op.line))
    d = _nchw(op, "out")
    _same(op, names, d)
    return BckOpShape(op.type, *d, n_ins=n_ins)


def sgemm_shape(op):
    if op.type != "sgemm":
        raise ValueError("not an sgemm op: %s" % op.type)
    a, b, c = op.dims["a"], op.dims["b"], op.dims["c"]
    s = SgemmShape(M=a["M"], N=b["N"], K=a["K"])
    if b["K"] != s.K or c["M"] != s.M or c["N"] != s.N:
        raise ValueError("sgemm dims inconsistent: %s" % op.line)
    return s


def read_ops(path, types=("Convolution", "sgemm")):
    """Read an op-list file. Returns (ops, skipped) where skipped counts lines of other types."""
    ops, skipped = [], 0
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            op = parse_op(line)
            if op.type not in types:
                skipped += 1
                continue
            ops.append(op)
    return ops, skipped


def shape_of(op):
    if op.type == "BckConv":
        return bck_conv_shape(op)
    if op.type == "Spreading":
        return spreading_shape(op)
    if op.type == "BckLRN":
        return bck_lrn_shape(op)
    if op.type == "SoftmaxWithLoss":
        return softmax_loss_shape(op)
    if op.type in ELEMENTWISE:
        return elementwise_shape(op)
    return conv_shape(op) if op.type == "Convolution" else sgemm_shape(op)
