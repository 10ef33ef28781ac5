// op_desc.cc -- see op_desc.H
#include "op_desc.H"

#include <algorithm>
#include <fstream>

#include "lexp.H"

namespace boda_hip {

std::string dims_t::str() const {
  std::string o = "(";
  if (tn != "float") o += "tn=" + tn + ",";
  o += "dims=(";
  for (size_t i = 0; i < d.size(); ++i) o += (i ? "," : "") + d[i].name + "=" + std::to_string(d[i].sz);
  return o + "))";
}

namespace {
dims_t dims_from_lexp(lexp_t const &l, std::string const &tn) {
  std::vector<std::pair<std::string, uint32_t>> nd;
  std::string t = tn;
  for (auto const &k : l.kids) {
    if (k.first == "__tn__") {
      t = k.second->leaf;
      continue;
    }
    if (k.second->is_list) rt_err("nested list where a dimension size was expected");
    nd.emplace_back(k.first, parse_u32(k.second->leaf, "dim size"));
  }
  return dims_t(nd, t);
}
}  // namespace

op_base_t parse_op_line(std::string const &line) {
  p_lexp_t t = parse_lexp(line);
  if (!t->is_list) rt_err("op line is not a list: " + line);
  op_base_t op;
  op.line = line;
  p_lexp_t sv = t->find("str_vals"), nv = t->find("nda_vals");
  if (nv || (sv && sv->is_list && sv->find("type"))) {  // current dialect
    for (auto const &k : t->kids)
      if (k.first != "str_vals" && k.first != "nda_vals") rt_err("unused input: " + k.first);
    if (!sv || !sv->find("type")) rt_err("op line without str_vals.type: " + line);
    for (auto const &k : sv->kids) {
      if (k.first == "type") op.type = k.second->leaf;
      else if (k.first == "func_name") op.func_name = k.second->leaf;
      else op.str_vals[k.first] = k.second->leaf;
    }
    if (nv)
      for (auto const &k : nv->kids) {
        lexp_t const &n = *k.second;
        p_lexp_t tn = n.find("tn"), dims = n.find("dims"), v = n.find("v");
        std::string tns = tn ? tn->leaf : "float";
        if (dims) op.dims_vals[k.first] = dims_from_lexp(*dims, tns);
        else if (v) op.scalars[k.first] = parse_u64(v->leaf, "scalar " + k.first);
        else rt_err("nda '" + k.first + "' has neither dims nor v");
      }
    return op;
  }
  p_lexp_t ty = t->find("type");  // legacy dialect
  if (!ty) rt_err("unrecognised op line: " + line);
  op.type = ty->leaf;
  for (auto const &k : t->kids) {
    if (k.first == "type") continue;
    if (k.first == "dims_vals") {
      for (auto const &d : k.second->kids) op.dims_vals[d.first] = dims_from_lexp(*d.second, "float");
    } else if (k.first == "str_vals") {
      for (auto const &s : k.second->kids) {
        std::string const &v = s.second->leaf;
        bool num = !v.empty() && std::all_of(v.begin(), v.end(), ::isdigit);
        if (num) op.scalars[s.first] = parse_u64(v, "scalar " + s.first);
        else op.str_vals[s.first] = v;
      }
    } else {
      rt_err("unused input: " + k.first);
    }
  }
  // legacy dims-only ndas carry no element type: kern_sz / stride / in_pad are 'none'
  for (char const *n : {"kern_sz", "stride", "in_pad"})
    if (op.dims_vals.count(n)) op.dims_vals[n].tn = "none";
  return op;
}

std::vector<op_base_t> read_op_list(std::string const &fn, size_t *skipped, std::vector<std::string> const &types) {
  std::ifstream f(fn);
  if (!f) rt_err("cannot open op list '" + fn + "'");
  std::vector<op_base_t> out;
  std::string line;
  size_t sk = 0;
  while (std::getline(f, line)) {
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
    if (line.empty()) continue;
    op_base_t op = parse_op_line(line);
    if (std::find(types.begin(), types.end(), op.type) == types.end()) {
      ++sk;
      continue;
    }
    out.push_back(op);
  }
  if (skipped) *skipped = sk;
  return out;
}

uint32_t conv_in_sz_to_out_sz(uint32_t in, uint32_t pad, uint32_t k, uint32_t stride) {
  uint32_t p = in + 2 * pad;
  if (p < k) return 0;
  return (p - k) / stride + 1;
}

conv_shape_t get_conv_shape(op_base_t const &op) {
  if (op.type != "Convolution") rt_err("not a Convolution op: " + op.type);
  dims_t const &in = op.get_dims("in"), &f = op.get_dims("filts");
  dims_t const &ks = op.get_dims("kern_sz"), &st = op.get_dims("stride"), &pd = op.get_dims("in_pad");
  conv_shape_t s;
  s.B = in.dsz("img"); s.IC = in.dsz("chan"); s.H = in.dsz("y"); s.W = in.dsz("x");
  s.OC = f.dsz("out_chan"); s.KY = ks.dsz("y"); s.KX = ks.dsz("x");
  s.sy = st.dsz("y"); s.sx = st.dsz("x"); s.py = pd.dsz("y"); s.px = pd.dsz("x");
  s.OH = conv_in_sz_to_out_sz(s.H, s.py, s.KY, s.sy);
  s.OW = conv_in_sz_to_out_sz(s.W, s.px, s.KX, s.sx);
  if (f.dsz("in_chan") != s.IC || f.dsz("y") != s.KY || f.dsz("x") != s.KX)
    rt_err("filts dims inconsistent with in / kern_sz: " + op.line);
  if (op.has_dims("out")) {
    dims_t const &o = op.get_dims("out");
    if (o.dsz("img") != s.B || o.dsz("chan") != s.OC || o.dsz("y") != s.OH || o.dsz("x") != s.OW)
      rt_err("out dims inconsistent with conv_in_sz_to_out_sz: " + op.line);
  }
  auto oc = op.scalars.find("out_chans");
  if (oc != op.scalars.end() && oc->second != s.OC) rt_err("out_chans mismatch: " + op.line);
  return s;
}

conv_shape_t get_bck_conv_shape(op_base_t const &op) {
  if (op.type != "BckConv") rt_err("not a BckConv op: " + op.type);
  dims_t const &in = op.get_dims("in"), &f = op.get_dims("filts"), &b = op.get_dims("biases");
  dims_t const &ks = op.get_dims("kern_sz"), &st = op.get_dims("stride"), &pd = op.get_dims("in_pad");
  conv_shape_t s;
  s.B = in.dsz("img"); s.IC = in.dsz("chan"); s.H = in.dsz("y"); s.W = in.dsz("x");
  s.OC = f.dsz("out_chan"); s.KY = ks.dsz("y"); s.KX = ks.dsz("x");
  s.sy = st.dsz("y"); s.sx = st.dsz("x"); s.py = pd.dsz("y"); s.px = pd.dsz("x");
  s.OH = conv_in_sz_to_out_sz(s.H, s.py, s.KY, s.sy);
  s.OW = conv_in_sz_to_out_sz(s.W, s.px, s.KX, s.sx);
  if (f.dsz("in_chan") != s.IC || f.dsz("y") != s.KY || f.dsz("x") != s.KX)
    rt_err("filts dims inconsistent with in / kern_sz: " + op.line);
  if (b.d.size() != 1 || b.d[0].sz != s.OC) rt_err("biases dims inconsistent with filts: " + op.line);
  // each gradient has the dims of the var it is the gradient of
  for (auto const &gv : {std::make_pair("in_grad_loss", "in"), std::make_pair("filts_grad_loss", "filts"),
                         std::make_pair("biases_grad_loss", "biases")})
    if (op.has_dims(gv.first) && op.get_dims(gv.first).str() != op.get_dims(gv.second).str())
      rt_err(std::string(gv.first) + " dims differ from " + gv.second + ": " + op.line);
  dims_t const &o = op.get_dims("out_grad_loss");
  if (o.dsz("img") != s.B || o.dsz("chan") != s.OC || o.dsz("y") != s.OH || o.dsz("x") != s.OW)
    rt_err("out_grad_loss dims inconsistent with conv_in_sz_to_out_sz: " + op.line);
  return s;
}

sgemm_shape_t get_sgemm_shape(op_base_t const &op) {
  if (op.type != "sgemm") rt_err("not an sgemm op: " + op.type);
  dims_t const &a = op.get_dims("a"), &b = op.get_dims("b"), &c = op.get_dims("c");
  sgemm_shape_t s{a.dsz("M"), b.dsz("N"), a.dsz("K")};
  if (b.dsz("K") != s.K || c.dsz("M") != s.M || c.dsz("N") != s.N) rt_err("sgemm dims inconsistent: " + op.line);
  if (a.tn != "float" || b.tn != "float" || c.tn != "float")
    unsup_err("hip backend sgemm is fp32 only (half-storage sgemm is out of scope)");
  return s;
}

uint32_t pool_in_sz_to_out_sz(uint32_t in, uint32_t pad, uint32_t k, uint32_t stride) {
  uint32_t p = in + 2 * pad;
  if (p < k) return 1;
  return (p - k + stride - 1) / stride + 1;
}

bool is_bck_op_type(std::string const &t) {
  return t == "Spreading" || t == "BckLRN" || t == "ZeroIfNonPos" || t == "BckDropout" || t == "Reduce" ||
         t == "SoftmaxWithLoss";
}

namespace {
struct nchw_t {
  uint32_t v[4];
  bool operator!=(nchw_t const &o) const { return !std::equal(v, v + 4, o.v); }
};
nchw_t get_nchw(op_base_t const &op, std::string const &n) {
  dims_t const &d = op.get_dims(n);
  char const *names[4] = {"img", "chan", "y", "x"};
  if (d.d.size() != 4) rt_err(n + " is not img x chan x y x x: " + op.line);
  nchw_t r;
  for (int i = 0; i < 4; ++i) {
    if (d.d[i].name != names[i]) rt_err(n + " is not img x chan x y x x: " + op.line);
    r.v[i] = d.d[i].sz;
  }
  return r;
}
void check_same(op_base_t const &op, std::vector<std::string> const &names, nchw_t const &want) {
  for (auto const &n : names)
    if (get_nchw(op, n) != want) rt_err(n + " dims differ from the op's geometry: " + op.line);
}
uint32_t scalar_or(op_base_t const &op, std::string const &n, uint32_t dflt) {
  auto it = op.scalars.find(n);
  return it == op.scalars.end() ? dflt : (uint32_t)it->second;
}
}  // namespace

bck_op_shape_t get_bck_op_shape(op_base_t const &op) {
  bck_op_shape_t s;
  std::string const &t = op.type;
  if (!is_bck_op_type(t)) rt_err("not a backward op of a non-conv layer: " + t);
  nchw_t d = get_nchw(op, t == "Spreading" || t == "BckLRN" || t == "SoftmaxWithLoss" ? "in" : "out");
  s.B = d.v[0]; s.C = d.v[1]; s.H = d.v[2]; s.W = d.v[3];
  if (t == "Spreading") {
    dims_t const &st = op.get_dims("stride"), &pd = op.get_dims("in_pad");
    s.KY = s.H; s.KX = s.W;  // no kern_sz: global pooling
    if (op.has_dims("kern_sz")) { s.KY = op.get_dims("kern_sz").dsz("y"); s.KX = op.get_dims("kern_sz").dsz("x"); }
    s.sy = st.dsz("y"); s.sx = st.dsz("x"); s.py = pd.dsz("y"); s.px = pd.dsz("x");
    s.avg = scalar_or(op, "avg_pool", 0);
    if (!s.KY || !s.KX || !s.sy || !s.sx) rt_err("zero kern_sz or stride: " + op.line);
    s.OH = pool_in_sz_to_out_sz(s.H, s.py, s.KY, s.sy);
    s.OW = pool_in_sz_to_out_sz(s.W, s.px, s.KX, s.sx);
    check_same(op, {"in_grad_loss"}, d);
    nchw_t o{{s.B, s.C, s.OH, s.OW}};
    check_same(op, {"out_grad_loss"}, o);
    if (op.has_dims("out")) check_same(op, {"out"}, o);
  } else if (t == "BckLRN") {
    check_same(op, {"out", "out_grad_loss", "in_grad_loss"}, d);
    if (!op.scalars.count("local_size")) rt_err("BckLRN op without local_size: " + op.line);
    s.local_size = scalar_or(op, "local_size", 0);
  } else if (t == "SoftmaxWithLoss") {
    check_same(op, {"in_grad_loss"}, d);
    dims_t want_label({{"img", s.B}, {"y", s.H}, {"x", s.W}}), want_loss({{"y", s.H}, {"x", s.W}});
    if (op.get_dims("label").str() != want_label.str()) rt_err("label dims inconsistent with in: " + op.line);
    if (op.get_dims("loss").str() != want_loss.str()) rt_err("loss dims inconsistent with in: " + op.line);
  } else if (t == "Reduce") {
    std::vector<std::string> names{"out"};
    while (op.has_dims("ins_" + std::to_string(s.n_ins))) names.push_back("ins_" + std::to_string(s.n_ins++));
    if (!s.n_ins || op.dims_vals.size() != s.n_ins + 1) rt_err("Reduce op needs ins_0 .. ins_n-1 and out: " + op.line);
    check_same(op, names, d);
  } else {
    std::vector<std::string> names{"in", "out"};
    if (t == "ZeroIfNonPos") names.push_back("cond");
    if (op.dims_vals.size() != names.size()) rt_err(t + " op lists other tensors than its own: " + op.line);
    check_same(op, names, d);
  }
  return s;
}

op_work_t op_work(op_base_t const &op) {
  op_work_t w;
  if (is_bck_op_type(op.type)) {
    // bytes = 4 x the elements of every tensor the definition reads or writes (boda_hip/ops.py BckOpShape
    // states the same model)
    bck_op_shape_t s = get_bck_op_shape(op);
    double N = s.N(), P = (double)s.B * s.H * s.W;
    if (op.type == "Spreading") {  // flops: the windows that can cover a pixel
      w.flops = N * ((s.KY + s.sy - 1) / s.sy) * ((s.KX + s.sx - 1) / s.sx);
      w.bytes = 4.0 * ((s.avg ? 1.0 : 2.0) * s.B * s.C * s.OH * s.OW + N);
    } else if (op.type == "BckLRN") {
      w.flops = N * (s.local_size + 8);
      w.bytes = 4.0 * 5 * N;
    } else if (op.type == "SoftmaxWithLoss") {
      w.flops = 3 * N;
      w.bytes = 4.0 * (3 * N + 2 * P + (double)s.H * s.W);
    } else if (op.type == "Reduce") {
      w.flops = s.n_ins * N;
      w.bytes = 4.0 * (s.n_ins + 1) * N;
    } else if (op.type == "BckDropout") {
      w.flops = N;
      w.bytes = 4.0 * 2 * N;
    } else {  // ZeroIfNonPos
      w.flops = 0;
      w.bytes = 4.0 * 3 * N;
    }
  } else if (op.type == "Split") {  // in read once, the outs (as many elements) written
    w.bytes = 4.0 * 2 * op.get_dims("in").elems();
  } else if (op.type == "Convolution") {
    conv_shape_t s = get_conv_shape(op);
    double M = (double)s.B * s.OH * s.OW, K = (double)s.IC * s.KY * s.KX, N = s.OC;
    w.flops = 2 * M * N * K;
    w.bytes = 4.0 * ((double)s.B * s.IC * s.H * s.W + (double)s.B * s.OC * s.OH * s.OW + N * K + N);
  } else if (op.type == "BckConv") {
    // the reference gives BckConv no single value (src/cnn_op.cc:330); ours: the input and the filter
    // gradient each do the forward's M*N*K multiply-adds, the bias gradient M*N adds; in and filts are
    // read and their gradients written, out_grad_loss read, biases_grad_loss written
    conv_shape_t s = get_bck_conv_shape(op);
    double M = (double)s.B * s.OH * s.OW, K = (double)s.IC * s.KY * s.KX, N = s.OC;
    w.flops = 4 * M * N * K + M * N;
    w.bytes = 4.0 * (2.0 * s.B * s.IC * s.H * s.W + 2 * N * K + M * N + N);
  } else if (op.type == "sgemm") {
    sgemm_shape_t s = get_sgemm_shape(op);
    w.flops = 2.0 * s.M * s.N * s.K;
    w.bytes = 4.0 * ((double)s.M * s.K + (double)s.K * s.N + (double)s.M * s.N);
  } else {
    rt_err("op_work: unhandled op type " + op.type);
  }
  return w;
}

double roofline_secs(op_work_t const &w) { return std::max(w.flops / PEAK_FP32_FLOPS, w.bytes / PEAK_HBM_BPS); }

void add_hip_annotations(op_base_t &op) {
  if (op.type == "Convolution") {
    conv_shape_t s = get_conv_shape(op);
    op.func_name = "hip_conv";
    op.dims_vals["in"] = dims_t({{"img", s.B}, {"chan", s.IC}, {"y", s.H}, {"x", s.W}});
    op.dims_vals["filts"] = dims_t({{"out_chan", s.OC}, {"in_chan", s.IC}, {"y", s.KY}, {"x", s.KX}});
    op.dims_vals["biases"] = dims_t({{"out_chan", s.OC}});
    op.dims_vals["out"] = dims_t({{"img", s.B}, {"chan", s.OC}, {"y", s.OH}, {"x", s.OW}});
    if (op.str_vals.count("conv_has_relu") == 0 && op.scalars.count("conv_has_relu") == 0)
      op.scalars["conv_has_relu"] = 1;  // ops-prof always fuses ReLU (src/cnn_op.cc:335-337)
    return;
  }
  if (op.type == "BckConv") {
    conv_shape_t s = get_bck_conv_shape(op);
    op.func_name = "hip_bck_conv";
    for (char const *n : {"in", "in_grad_loss"})
      op.dims_vals[n] = dims_t({{"img", s.B}, {"chan", s.IC}, {"y", s.H}, {"x", s.W}});
    for (char const *n : {"filts", "filts_grad_loss"})
      op.dims_vals[n] = dims_t({{"out_chan", s.OC}, {"in_chan", s.IC}, {"y", s.KY}, {"x", s.KX}});
    for (char const *n : {"biases", "biases_grad_loss"}) op.dims_vals[n] = dims_t({{"out_chan", s.OC}});
    op.dims_vals["out_grad_loss"] = dims_t({{"img", s.B}, {"chan", s.OC}, {"y", s.OH}, {"x", s.OW}});
    return;
  }
  if (op.type == "sgemm") {
    get_sgemm_shape(op);
    op.func_name = "hip_sgemm";
    return;
  }
  if (is_bck_op_type(op.type)) {
    // the vars of the .cucl definitions (test/rtc/{spreading,bck_lrn,ZeroIfNonPos,reduce,dropout}.cucl and
    // the three calls of SoftmaxWithLoss), those the forward op makes (out_in_yx, out_scale_base) included
    bck_op_shape_t s = get_bck_op_shape(op);
    const dims_t full({{"img", s.B}, {"chan", s.C}, {"y", s.H}, {"x", s.W}});
    if (op.type == "Spreading") {
      op.func_name = "hip_spreading";
      const dims_t o({{"img", s.B}, {"chan", s.C}, {"y", s.OH}, {"x", s.OW}});
      for (char const *n : {"out", "out_grad_loss", "out_in_yx"}) op.dims_vals[n] = o;
      // hip_pool's geometry names, so the op also describes the forward call that makes out_in_yx
      op.scalars["ky"] = s.KY; op.scalars["kx"] = s.KX; op.scalars["sy"] = s.sy; op.scalars["sx"] = s.sx;
      op.scalars["py"] = s.py; op.scalars["px"] = s.px; op.scalars["avg"] = s.avg;
    } else if (op.type == "BckLRN") {
      op.func_name = "hip_bck_lrn";
      op.dims_vals["out_scale_base"] = full;
    } else if (op.type == "ZeroIfNonPos") {
      op.func_name = "hip_zero_if_non_pos";
    } else if (op.type == "BckDropout") {  // in place, and its own backward
      op.func_name = "hip_dropout";
      op.dims_vals["inout"] = full;
    } else if (op.type == "Reduce") {
      op.func_name = "hip_reduce";
      op.scalars["ins_num"] = s.n_ins;
    } else {
      op.func_name = "hip_softmax_with_loss";
      op.dims_vals["prob"] = full;
      op.dims_vals["loss_per_pel"] = op.get_dims("label");
    }
    return;
  }
  if (op.type == "Split") {  // one hip_copy per outs_<i>, its channels taken in order from in
    dims_t const &in = op.get_dims("in");
    uint32_t n = 0, chans = 0;
    for (; op.has_dims("outs_" + std::to_string(n)); ++n) {
      dims_t const &o = op.get_dims("outs_" + std::to_string(n));
      if (o.dsz("img") != in.dsz("img") || o.dsz("y") != in.dsz("y") || o.dsz("x") != in.dsz("x"))
        rt_err("Split: outs_" + std::to_string(n) + " differs from in outside chan: " + op.line);
      chans += o.dsz("chan");
    }
    if (!n || chans != in.dsz("chan")) rt_err("Split: the outs' channels do not add up to in's: " + op.line);
    op.func_name = "hip_copy";
    op.scalars["outs_num"] = n;
    return;
  }
  unsup_err("hip backend: no kernel for op type '" + op.type + "'");
}

std::string hip_op_tune_t::str() const {
  std::string r;
  auto add = [&](std::string const &k, std::string const &v) { r += (r.empty() ? "" : ",") + k + "=" + v; };
  if (!use_be.empty()) add("use_be", use_be);
  if (!cfg.empty()) add("cfg", cfg);
  if (splits) add("splits", std::to_string(splits));
  if (wt >= 0) add("wt", std::to_string(wt));
  return "(" + r + ")";
}

hip_op_tune_t parse_hip_op_tune(std::string const &s) {
  p_lexp_t l = parse_lexp(s);
  hip_op_tune_t t;
  if (!l->is_list) rt_err("op_tune: expected a (k=v,...) list, got '" + s + "'");
  for (auto const &kv : l->kids) {
    if (kv.second->is_list) rt_err("op_tune: field '" + kv.first + "' is a list");
    std::string const &v = kv.second->leaf;
    try {
      if (kv.first == "use_be") t.use_be = v;
      else if (kv.first == "cfg") t.cfg = v;
      else if (kv.first == "splits") t.splits = parse_i32(v, "splits");
      else if (kv.first == "wt") t.wt = parse_i32(v, "wt");
      else rt_err("op_tune: unknown field '" + kv.first + "' (use_be, cfg, splits, wt)");
    } catch (std::logic_error const &) {
      rt_err("op_tune: bad value '" + v + "' for " + kv.first);
    }
  }
  if (!t.use_be.empty() && t.use_be != "hip") unsup_err("op_tune: use_be=" + t.use_be + " is not this backend");
  if (t.wt < -1 || t.wt > 1) rt_err("op_tune: wt must be -1, 0 or 1");
  return t;
}

void add_hip_annotations(op_base_t &op, hip_op_tune_t const &tune) {
  add_hip_annotations(op);
  if (!tune.cfg.empty()) op.str_vals["hip_cfg"] = tune.cfg;
  if (tune.splits) op.str_vals["hip_splits"] = std::to_string(tune.splits);
  if (tune.wt >= 0) op.str_vals["hip_wt"] = std::to_string(tune.wt);
}

}  // namespace boda_hip
