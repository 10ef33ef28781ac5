"""The library's routes, GPU-free: the ordered configuration lists of sgemm and conv (tools and tests
pass positional indices to bh_tune_set), the variant bh_variant_name gives every shape of the tuning
table, every conv / sgemm op of three op lists and a handful of off-table shapes that reach each branch
of the heuristic, and the Winograd bank bh_conv_route_banks names for the table's 3x3 / 5x5 lines.

tests/golden/routes/routes.txt records them as the library answered BEFORE cfg_t became a tagged
struct; the test asserts the library still answers the same, line for line. The file is regenerated
only on purpose, from a library known to be right: python tests/test_routes_cpu.py (with BH_LIB_NAME
naming the build to record, see boda_hip/__init__.py)."""
import ctypes
import os

import boda_hip
from boda_hip import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = os.path.join(ROOT, "tests", "golden", "ops")
TUNE = os.path.join(ROOT, "boda-1_amd", "tuning", "gfx950.tune")
FIXTURE = os.path.join(ROOT, "tests", "golden", "routes", "routes.txt")
OP_LISTS = ("conv-ops-1-5-20-nin-alex-gn", "op_sigs_full", "sgemm-ops-full")

# off-table shapes, one per branch of the heuristic (bh_gemm.hip heuristic()); conv dims are
# B IC H W OC KY KX sy sx py px, sgemm dims M N K
OFF_TABLE = (
    ("gv N<=16", 1, (1, 512, 7, 7, 1024, 7, 7, 1, 1, 0, 0)),
    ("gv N<=32", 1, (2, 1024, 4, 4, 1024, 1, 1, 1, 1, 0, 0)),
    ("gv N<=64", 1, (4, 1024, 4, 4, 1024, 1, 1, 1, 1, 0, 0)),
    ("gv shape with K%4", 1, (1, 1023, 4, 4, 1100, 1, 1, 1, 1, 0, 0)),
    ("N<=32", 1, (1, 16, 4, 4, 64, 3, 3, 1, 1, 1, 1)),
    ("OC<=32", 1, (1, 16, 20, 20, 24, 3, 3, 1, 1, 1, 1)),
    ("ring 128x128", 1, (8, 64, 64, 64, 256, 3, 3, 1, 1, 1, 1)),
    ("ring OC<=64", 1, (1, 64, 40, 40, 48, 3, 3, 1, 1, 1, 1)),
    ("ring 64x64", 1, (1, 64, 40, 40, 96, 3, 3, 1, 1, 1, 1)),
    ("OC<=64", 1, (1, 8, 20, 20, 48, 3, 3, 1, 1, 1, 1)),
    ("128x32x32", 1, (1, 64, 20, 20, 96, 3, 3, 1, 1, 1, 1)),
    ("K%4", 1, (1, 3, 30, 30, 96, 3, 3, 1, 1, 1, 1)),
    ("default", 1, (4, 16, 64, 64, 128, 3, 3, 1, 1, 1, 1)),
    ("sgemm ring", 0, (2000, 3000, 1000)),
    ("sgemm tile", 0, (100, 100, 100)),
    ("sgemm scalar", 0, (1001, 1003, 777)),
    ("sgemm scalar big", 0, (4001, 4003, 1000)),
)


def table_lines():
    """(op kind, dims) of every shape line of the tuning table, in file order."""
    out = []
    with open(TUNE) as f:
        for line in f:
            w = line.split()
            if not w or w[0] not in ("conv", "sgemm"):
                continue
            n = 11 if w[0] == "conv" else 3
            out.append((1 if w[0] == "conv" else 0, tuple(int(x) for x in w[1:1 + n])))
    return out


def route_banks(dims):
    arr = (ctypes.c_uint32 * 16)(*dims)
    b = ctypes.c_uint32(0)
    assert boda_hip.lib().bh_conv_route_banks(None, arr, ctypes.byref(b)) == boda_hip.BH_OK
    return b.value


def routes():
    """The lines of the fixture, as the loaded library answers now."""
    out = []
    for op in (0, 1):
        out += ["cfg %d %d %s" % (op, i, n) for i, n in enumerate(boda_hip.tune_cfg_names(op))]

    def variant(tag, op, dims):
        out.append("%s | %d %s | %s" % (tag, op, " ".join(map(str, dims)), boda_hip.variant_name(op, dims)))

    table = table_lines()
    for op, dims in table:
        variant("tune", op, dims)
    for name in OP_LISTS:
        for o in ops.read_ops(os.path.join(OPS, name + ".txt"))[0]:
            s = ops.shape_of(o)
            if o.type == "sgemm":
                variant(name, 0, (s.M, s.N, s.K))
            else:
                variant(name, 1, s.as_dims())
    for tag, op, dims in OFF_TABLE:
        assert (op, tuple(dims)) not in table, tag
        variant("heuristic " + tag, op, dims)
    for op, dims in table:
        if op == 1 and dims[5] == dims[6] and dims[5] in (3, 5):
            out.append("banks | %s | %d" % (" ".join(map(str, dims)), route_banks(dims)))
    return out


def write_fixture():
    """Record the routes of the library in use (not called by the test)."""
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        f.write("\n".join(routes()) + "\n")


def test_routes_unchanged():
    with open(FIXTURE) as f:
        want = f.read().splitlines()
    got = routes()
    assert len(want) > 1000  # both config lists, the table, the op lists
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, diff[:10]
    assert len(got) == len(want)


if __name__ == "__main__":
    write_fixture()
