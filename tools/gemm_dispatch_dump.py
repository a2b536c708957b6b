#!/usr/bin/env python
"""What the GEMM / 3x3-conv and the attention host code decide for a fixed corpus of descriptors, one line per descriptor:

    <kind> <descriptor> -> <tile tile_m tile_n splitk workspace_bytes tail_rows stages> [| rc <rc> <error text> | <launch-log lines>]
    conv <descriptor> -> <plan as above> | <kernel symbol> splitk<n> [| rc ... | ...]      (e4t_conv3x3_kernel: what the launch will run)
    attn <shape> ws=<workspace offered> -> <forward kernel | dQ kernel | dK/dV kernel | tsplit tchunk | workspace_floats> [| rc ... | ...]

Two builds of the library (E4T_LIB=<path to libe4t_hip.so> selects another one) decide alike iff their dumps are byte-identical:

    python tools/gemm_dispatch_dump.py > new.txt;  E4T_LIB=/path/to/old/libe4t_hip.so python tools/gemm_dispatch_dump.py > old.txt;  diff old.txt new.txt

The plan half (e4t_gemm_plan / e4t_conv3x3_plan / e4t_gemm_tn_plan / e4t_attention_plan) is pure host code.  The launch half calls e4t_gemm_nt /
e4t_conv3x3 / e4t_gemm_tn / e4t_attention_fwd + e4t_attention_bwd_ws with FAKE operand pointers and the launch log on: the library writes the symbol | shape | bytes | flops line(s) of what it
would launch and then fails with "no ROCm-capable device".  That only works — and is only safe — on a machine WITHOUT a GPU: where a
device answers, the tool prints the plan half only and says so.  Environment switches of the library (E4T_GEMM_REGSTAGE,
E4T_CONV_NOSTRIP, ...) are read once per process: one run per setting.

    --plans            plan half only
    --group 'gemm t160'  only that corpus group (a group = one tile hint x {gemm, conv}, 'tn', 'attn', or 'step')
    --anchor           check the 'step' group against profiles/r06_roofline_per_shape.csv: every GEMM / conv / TN launch recorded there
                       on hardware is reproduced (symbol and shape string), every split-K reduce row by a launch's second log line
    --record           rewrite tests/gemm_dispatch_record.txt (what tests/test_gemm_dispatch.py compares against) from this library
    --conv-check       hold e4t_conv3x3_kernel against the launch log: for every conv item of the corpus and of conv_geometry_corpus() the symbol
                       and split-K of the query equal the first field and the splitk of the log line (or both refuse with the same code)
    --gemm-check       hold e4t_gemm_kernel / e4t_gemm_tn_kernel against the launch log: for every gemm and tn item of the corpus (the step table's
                       included) the symbol, the split-K and the reduce kernel of the query equal the first field and the splitk of the launch's
                       log line and the first field of its reduce line (or both refuse with the same code and text)
    --attn-launches    the 'attn' group as the launch log alone tells it (kernel symbols; workspace floats from
                       e4t_attention_bwd_workspace_floats): needs no e4t_attention_plan, so E4T_LIB may be a library older than that entry point
    --attn-check FILE  hold such a dump against e4t_attention_plan of this library; prints every row that differs (the record's 'attn' group
                       was anchored this way to the last commit before the plan existed)
"""
import argparse
import collections
import csv
import ctypes as C
import hashlib
import itertools
import os
import re
import sys
import tempfile

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "e4t-diffusion_amd")]
from e4t import _C  # noqa: E402

STEP_CSV = os.path.join(R, "profiles", "r06_roofline_per_shape.csv")
RECORD = os.path.join(R, "tests", "gemm_dispatch_record.txt")
FAKE = 1 << 24                       # a non-NULL, 16-byte aligned "pointer": never dereferenced by host code
OUT_F32, RES_F32, ACT_GELU, ACCUM, REDUCE_BATCH = 1, 2, 4, 8, 16
# 256, 640, 1128, 1160, 5064, 5128: codes of removed variants, kept as aliases (gemm.hip, decode_hint); 7: not a tile code
HINTS = [0, 64, 128, 160, 256, 512, 640, 1128, 1160, 2320, 3064, 3128, 3160, 4064, 4128, 4160, 5064, 5128, 5256, 7]
Item = collections.namedtuple("Item", "group kind kw")


def gemm_item(group, kind="gemm", **kw):
    return Item(group, kind, kw)


def conv_geometry(mode, H):
    """(Hin, Hout) of a consistent square problem"""
    return {1: (H, H), 2: (H, (H - 1) // 2 + 1), 3: (H, 2 * H), 4: (H, 2 * H), 5: (H, (H - 2) // 2 + 1)}[mode]


def step_rows():
    rows = [r for r in csv.reader(l for l in open(STEP_CSV) if not l.startswith("#"))][1:]
    return [(r[0], r[1]) for r in rows if re.match(r"gemm|conv_strip|splitk_reduce", r[0])]


def step_items():
    """The GEMM / conv / TN launches of the training step as profiles/r06_roofline_per_shape.csv recorded them.  Its shape string does not
    carry every descriptor field: each row comes with the combinations of the unrecorded ones (--anchor finds the one that was run)."""
    for sym, shape in step_rows():
        m = re.match(r"gemm M(\d+) N(\d+) K(\d+) batch(\d+) splitk(\d+) flags(\d+)$", shape)
        if m:
            M, N, K, b, _, fl = map(int, m.groups())
            for cs, (rb, rpb) in itertools.product((0, 1), ((0, 0), (1, 257), (1, 77))):
                yield Item("step", "gemm", dict(M=M, N=N, K=K, batch=b, flags=fl, colstats=cs, rowbias=rb, rows_per_batch=rpb, residual=1 if fl & RES_F32 else 0))
        m = re.match(r"conv mode(\d) (\d+)x(\d+)->(\d+)x(\d+) Cin(\d+) Cout(\d+) M(\d+) splitk(\d+)$", shape)
        if m:
            mode, Hi, Wi, Ho, Wo, Ci, Co, M, _ = map(int, m.groups())
            for cs in (0, 1):
                yield Item("step", "conv", dict(B=M // (Ho * Wo), Hin=Hi, Win=Wi, Cin=Ci, Hout=Ho, Wout=Wo, Cout=Co, mode=mode, colstats=cs))
        m = re.match(r"gemm_tn M(\d+) N(\d+) K(\d+) splitk(\d+) flags(\d+)$", shape)
        if m:
            M, N, K, _, fl = map(int, m.groups())
            yield Item("step", "tn", dict(M=M, N=N, K=K, flags=fl))


def corpus():
    yield from step_items()
    Ms = [16, 77, 257, 576, 1024, 1232, 2056, 4096, 4112, 4128, 4129, 16384, 65536]
    Ns = [64, 72, 128, 200, 320, 640, 768, 1000, 1280, 2560, 3840, 5120, 10240]
    Ks = [64, 72, 192, 320, 328, 640, 1280, 2560, 5120, 10240]
    flag_sets = [dict(flags=0), dict(flags=OUT_F32), dict(flags=OUT_F32 | RES_F32, residual=1), dict(flags=ACT_GELU), dict(flags=ACCUM | OUT_F32)]
    ms, ns, ks = [77, 1024, 4096, 4112, 65536], [128, 320, 1280, 2560], [64, 320, 1280, 10240]
    for t in HINTS:
        g = "gemm t%d" % t
        for M, N, K, sk, fl in itertools.product(Ms, Ns, Ks, [0, 1, 2, 3, 8], flag_sets):
            yield gemm_item(g, M=M, N=N, K=K, tile=t, splitk=sk, **fl)
        for M, N, K in itertools.product(ms, ns, ks):
            for rpb in (77, 96, 4096):
                yield gemm_item(g, M=M, N=N, K=K, tile=t, rowbias=1, rows_per_batch=rpb)
            for K1 in sorted({64, K // 128 * 64} - {0, K}):
                if K1 < K:
                    yield gemm_item(g, M=M, N=N, K=K, tile=t, A2=1, K1=K1, lda=K1, lda2=K - K1)
            for sk in (0, 1):
                yield gemm_item(g, M=M, N=N, K=K, tile=t, splitk=sk, colstats=1)
            if M % 256 == 0:
                yield gemm_item(g, M=M, N=N, K=K, tile=t, panel_rows=256, panel_stride=257, panel_off=1)
                yield gemm_item(g, M=M, N=N, K=K, tile=t, panel_rows=256, panel_stride=257, panel_off=1, flags=ACT_GELU)
            if M <= 4112:
                for b, fl in itertools.product((2, 129), (0, OUT_F32, REDUCE_BATCH | OUT_F32)):
                    yield gemm_item(g, M=M, N=N, K=K, tile=t, batch=b, flags=fl)
            for sk in (0, 3):      # the scalar epilogue and the scalar reduce
                yield gemm_item(g, M=M, N=N, K=K, tile=t, splitk=sk, ldc=N + 4)
                yield gemm_item(g, M=M, N=N, K=K, tile=t, splitk=sk, C_off=8)
                yield gemm_item(g, M=M, N=N, K=K, tile=t, splitk=sk, flags=OUT_F32, ldc=N + 2)
            for sk, ws in itertools.product((0, 3), ("none", "small")):      # automatic: one pass; explicit: -12
                yield gemm_item(g, M=M, N=N, K=K, tile=t, splitk=sk, ws=ws)
        yield gemm_item(g, M=1280, N=1280, K=8, tile=t, batch=129, flags=REDUCE_BATCH | OUT_F32)      # the E4T head's weight gradient
        for N in (320, 1280):      # an operand beyond 4 GB: the register-staged fallback
            yield gemm_item(g, M=1 << 20, N=N, K=4096, tile=t)
            yield gemm_item(g, M=1 << 20, N=N, K=4096, tile=t, flags=ACT_GELU)
    Cs = [64, 128, 256, 320, 512, 640, 1280, 2560]
    for t in HINTS:
        g = "conv t%d" % t
        for mode, B, H, Cin, Cout, sk in itertools.product((1, 2, 3, 4, 5), (1, 4, 16), (8, 16, 32, 64, 128), Cs, Cs, (0, 1, 3)):
            Hin, Hout = conv_geometry(mode, H)
            yield Item(g, "conv", dict(B=B, Hin=Hin, Win=Hin, Cin=Cin, Hout=Hout, Wout=Hout, Cout=Cout, mode=mode, tile=t, splitk=sk))
        for mode, B, H, Cin, Cout in itertools.product((1, 2, 3), (1, 16), (8, 32, 64), (128, 320, 1280), (128, 320, 512, 1280)):
            Hin, Hout = conv_geometry(mode, H)
            base = dict(B=B, Hin=Hin, Win=Hin, Cin=Cin, Hout=Hout, Wout=Hout, Cout=Cout, mode=mode, tile=t)
            yield Item(g, "conv", dict(base, flags=ACT_GELU))
            yield Item(g, "conv", dict(base, colstats=1, rowbias=1))
            yield Item(g, "conv", dict(base, flags=OUT_F32, residual=1))
            yield Item(g, "conv", dict(base, ws="none"))
            yield Item(g, "conv", dict(base, ws="small", splitk=3))
    for M, N, K, sk, fl, ws in itertools.product((64, 320, 960, 1280), (64, 320, 1280), (512, 4096, 65536, 1 << 20), (0, 1, 4, 32),
                                                 (dict(flags=0), dict(flags=OUT_F32), dict(flags=ACCUM | OUT_F32), dict(flags=RES_F32, residual=1)),
                                                 ("big", "none", "small")):
        yield Item("tn", "tn", dict(M=M, N=N, K=K, splitk=sk, ws=ws, **fl))
    yield from attn_corpus()


def conv_geometry_corpus():
    """what the square images of corpus() leave out: the strip predicates' widths (16 / 64 / 256 / 512) with and without whole 256-pixel tiles of rows,
    non-square images, a row bias over Hout * Wout % 32 != 0 pixels (the GENERAL epilogue), all five modes, every kernel family's tile hint,
    an input map beyond 4 GB"""
    def geo(mode, H, W):
        (Hin, Hout), (Win, Wout) = conv_geometry(mode, H), conv_geometry(mode, W)
        return dict(Hin=Hin, Win=Win, Hout=Hout, Wout=Wout)
    sizes = [(H, W) for W in (16, 64, 256, 512) for H in (1, 2, 3, 4, 6, 16)] + [(8, 8), (9, 9), (9, 7), (5, 5), (20, 12), (48, 40), (24, 24), (1, 7), (7, 1), (2, 2), (1, 1)]
    for t, mode, (H, W), B, (Cin, Cout) in itertools.product((0, 64, 3064, 4064, 128, 4128, 160, 3160, 512, 2320, 5256), (1, 2, 3, 4, 5), sizes, (1, 3),
                                                             ((64, 64), (64, 72), (128, 256), (192, 320), (64, 4))):
        if mode == 5 and (H < 2 or W < 2):
            continue
        base = dict(B=B, Cin=Cin, Cout=Cout, mode=mode, tile=t, **geo(mode, H, W))
        yield Item("conv geometry", "conv", base)
        yield Item("conv geometry", "conv", dict(base, rowbias=1, bias=1, residual=1))
        yield Item("conv geometry", "conv", dict(base, splitk=1, colstats=1))
        yield Item("conv geometry", "conv", dict(base, splitk=3))
        yield Item("conv geometry", "conv", dict(base, ws="none"))
        yield Item("conv geometry", "conv", dict(base, flags=OUT_F32))
    for t, mode in itertools.product((0, 64, 128, 512, 2320), (1, 2, 3, 4, 5)):      # an input map beyond 4 GB: the register-staged fallback
        yield Item("conv geometry", "conv", dict(B=16, Cin=512, Cout=320, mode=mode, tile=t, **geo(mode, 512, 512)))


ATTN_WS = ("full", "delta", "delta3", "short")      # the size the library asks for | B*H*T (Delta only) | B*H*T + 3 | one float short of the first


def attn_items(shapes):
    for B, H, T, S, DH, causal in shapes:
        for ws in ATTN_WS:
            yield Item("attn", "attn", dict(B=B, H=H, T=T, S=S, DH=DH, causal=causal, ws=ws))


def attn_step_shapes():
    """(B, H, T, S, DH, causal) of the attention launches profiles/r06_roofline_per_shape.csv recorded, and the kernel symbols seen for each"""
    seen = collections.OrderedDict()
    for l in open(STEP_CSV):
        m = re.match(r"(attn_\w+<(\d+)[^>]*>),B(\d+) H(\d+) T(\d+) S(\d+) causal(\d),", l)
        if m:
            B, H, T, S, c = map(int, m.groups()[2:])
            seen.setdefault((B, H, T, S, int(m.group(2)), c), []).append(m.group(1))
    return seen


def attn_corpus():
    """both sides of every threshold of the attention dispatch (S 192 / 512 / 2048, T 192 / 512, fewer than 512 dK/dV workgroups), each with the
    four workspace sizes; two rows around T * 8 = 2^31 (the DMA-staged dK/dV kernel's 32-bit extent of the {L, Delta} pairs)"""
    sizes = (1, 33, 77, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1024, 2047, 2048, 2050, 4096, 9216)
    shapes = [(B, H, T, S, DH, c) for DH, c, (B, H), T, S in itertools.product((32, 40, 64, 80, 160), (0, 1), ((1, 1), (2, 8), (4, 5), (16, 8)), sizes, sizes)]
    return attn_items(shapes + [(16, 8, (1 << 28) - 1, 512, 40, 0), (16, 8, 1 << 28, 512, 40, 0)])


def describe(kw):
    return " ".join("%s=%s" % kv for kv in kw.items())


def make_desc(item):
    """ctypes descriptor of a corpus item: dense row-major operands, FAKE wherever a pointer is wanted, a large workspace offered unless ws="""
    kw = dict(item.kw)
    ws = kw.pop("ws", "big")
    wskw = dict(workspace=None if ws == "none" else FAKE, workspace_bytes={"big": 1 << 40, "none": 0, "small": 16}[ws])
    ptr = lambda name: FAKE if kw.pop(name, 0) else None
    if item.kind == "conv":
        return _C.ConvDesc(X=FAKE, W=FAKE, Y=FAKE, bias=ptr("bias"), residual=ptr("residual"), rowbias=ptr("rowbias"), colstats=ptr("colstats"), **wskw, **kw)
    M, N, K = kw["M"], kw["N"], kw["K"]
    base = dict(A=FAKE, B=FAKE, C=FAKE + kw.pop("C_off", 0), A2=ptr("A2"), bias=ptr("bias"), residual=ptr("residual"), rowbias=ptr("rowbias"), colstats=ptr("colstats"),
                K1=K, lda=K, ldb=K, ldc=N, ldr=N, batch=1, alpha=1.0, strideA=M * K, strideB=N * K, strideC=M * N)
    if item.kind == "tn":
        base.update(lda=M, ldb=N, strideA=0, strideB=0, strideC=0)
    base.update(wskw)
    base.update(kw)
    return _C.GemmDesc(**base)


def load_lib():
    """the library through e4t._C; a build from before e4t_attention_plan (E4T_LIB, for --attn-launches) through plain ctypes with the signatures it has"""
    try:
        return _C.load()
    except AttributeError:
        lib = C.CDLL(_C.LIB_PATH)
        for name, (res, args) in _C.SIGNATURES.items():
            if hasattr(lib, name):
                getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
        return lib


class Dumper:
    def __init__(self, launches):
        self.lib = load_lib()
        self.plan_fn = {"gemm": self.lib.e4t_gemm_plan, "conv": self.lib.e4t_conv3x3_plan, "tn": self.lib.e4t_gemm_tn_plan}
        self.launch_fn = {"gemm": self.lib.e4t_gemm_nt, "conv": self.lib.e4t_conv3x3, "tn": self.lib.e4t_gemm_tn}
        self.log = None
        if launches:
            fd, self.log_path = tempfile.mkstemp(suffix=".launchlog")
            os.close(fd)
            assert self.lib.e4t_set_launch_log(self.log_path.encode()) == 0
            self.log = open(self.log_path)

    def close(self):
        if self.log:
            self.lib.e4t_set_launch_log(None)
            self.log.close()
            os.remove(self.log_path)

    def attn_ws(self, kw):
        shape = [kw[k] for k in ("B", "H", "T", "S", "DH")]
        full, delta = self.lib.e4t_attention_bwd_workspace_floats(*shape), kw["B"] * kw["H"] * kw["T"]
        return shape, {"full": full, "delta": delta, "delta3": delta + 3, "short": full - 1}[kw["ws"]]

    def attn_plan(self, kw):
        shape, ws = self.attn_ws(kw)
        pl = _C.AttentionPlan()
        rc = self.lib.e4t_attention_plan(*shape, kw["causal"], ws, C.byref(pl))
        if rc != 0:
            return "rc %d %s" % (rc, self.lib.e4t_last_error().decode())
        return "%s | %s | %s | %d %d | %d" % (pl.fwd.decode(), pl.dq.decode(), pl.dkv.decode(), pl.tsplit, pl.tchunk, pl.workspace_floats)

    def attn_launch(self, kw):
        """(rc of the backward, its error text, the log lines of forward + backward); dense q | k | v rows"""
        (B, H, T, S, DH), ws = self.attn_ws(kw)
        ld = H * DH
        tail = [B, H, T, S, DH, ld, ld, ld, ld, T * ld, S * ld, S * ld, T * ld, C.c_float(DH ** -0.5), kw["causal"], None]
        self.lib.e4t_attention_fwd(FAKE, FAKE, FAKE, FAKE, FAKE, *tail)
        rc = self.lib.e4t_attention_bwd_ws(*[FAKE] * 7, ws, FAKE, FAKE, FAKE, *tail)
        return rc, (self.lib.e4t_last_error().decode() if rc < 0 else ""), self.log.read().splitlines()

    def plan(self, item, d=None):
        if item.kind == "attn":
            return self.attn_plan(item.kw)
        d = d or make_desc(item)
        pl = _C.GemmPlan()
        rc = self.plan_fn[item.kind](C.byref(d), C.byref(pl))
        if rc != 0:
            return "rc %d %s" % (rc, self.lib.e4t_last_error().decode())
        return "%d %d %d %d %d %d %d" % (pl.tile, pl.tile_m, pl.tile_n, pl.splitk, pl.workspace_bytes, pl.tail_rows, pl.stages)

    def conv_kernel(self, item, d=None):
        """what e4t_conv3x3_kernel says the launch of a conv item will run: "<kernel symbol> splitk<n>" (pure host code, like the plan)"""
        sym, sk = C.c_char_p(), C.c_int(0)
        rc = self.lib.e4t_conv3x3_kernel(C.byref(d or make_desc(item)), C.byref(sym), C.byref(sk))
        if rc != 0:
            return "rc %d %s" % (rc, self.lib.e4t_last_error().decode())
        return "%s splitk%d" % (sym.value.decode(), sk.value)

    def gemm_kernel(self, item, d=None):
        """what e4t_gemm_kernel / e4t_gemm_tn_kernel say the launch of a gemm / tn item will run:
        "<kernel symbol> splitk<n> <store path> [<reduce symbol>] [tail<r>] [colstats]" (pure host code, like the plan)"""
        k = _C.GemmKernel()
        rc = (self.lib.e4t_gemm_kernel if item.kind == "gemm" else self.lib.e4t_gemm_tn_kernel)(C.byref(d or make_desc(item)), C.byref(k))
        if rc != 0:
            return "rc %d %s" % (rc, self.lib.e4t_last_error().decode())
        return " ".join(["%s splitk%d %s" % (k.symbol.decode(), k.splitk, _C.STORE_NAMES[k.store])] + ([k.reduce.decode()] if k.reduce else []) +
                        (["tail%d" % k.tail_rows] if k.tail_rows else []) + (["colstats"] if k.colstats else []))

    def launch(self, item, d=None):
        """(rc, error text, [log lines])"""
        if item.kind == "attn":
            return self.attn_launch(item.kw)
        d = d or make_desc(item)
        rc = self.launch_fn[item.kind](C.byref(d), None)
        return rc, (self.lib.e4t_last_error().decode() if rc < 0 else ""), self.log.read().splitlines()

    def line(self, item):
        d = None if item.kind == "attn" else make_desc(item)
        s = "%s %s -> %s" % (item.kind, describe(item.kw), self.plan(item, d))
        if item.kind == "conv" and hasattr(self.lib, "e4t_conv3x3_kernel"):
            s += " | " + self.conv_kernel(item, d)
        if self.log:
            rc, err, lines = self.launch(item, d)
            s += " | rc %d %s | %s" % (rc, err, " ; ".join(lines))
        return s


def gpu_visible(lib):
    n = C.c_int(0)
    return lib.e4t_device_info(None, 0, C.byref(n)) == 0


def plan_digests(dumper):
    """{group: (lines, sha256 of the plan half)} in corpus order, and the plan lines of the 'step' group"""
    h, n, step = collections.OrderedDict(), collections.Counter(), []
    for item in corpus():
        s = "%s %s -> %s" % (item.kind, describe(item.kw), dumper.plan(item))
        h.setdefault(item.group, hashlib.sha256()).update((s + "\n").encode())
        n[item.group] += 1
        if item.group == "step":
            step.append(s)
    return collections.OrderedDict((g, (n[g], h[g].hexdigest())) for g in h), step


def anchor(dumper):
    """every launch row of the step table is reproduced by one of its field combinations; every reduce row by a second log line"""
    want = step_rows()
    got, matched = collections.defaultdict(list), []
    for item in step_items():
        rc, err, lines = dumper.launch(item)
        for i, l in enumerate(lines):
            got[tuple(l.split("|")[:2])].append((i, item))
    miss = 0
    for sym, shape in want:
        hits = [it for i, it in got.get((sym, shape), []) if (i == 1) == sym.startswith("splitk_reduce")]
        if hits:
            matched.append((sym, shape, hits[0]))
        else:
            miss += 1
            print("MISS %s|%s" % (sym, shape))
    launches = sum(1 for s, _ in want if not s.startswith("splitk_reduce"))
    print("step table: %d rows (%d launches, %d reduces), %d reproduced, %d missed" % (len(want), launches, len(want) - launches, len(matched), miss))
    return matched, miss


def conv_check(dumper):
    """rows on which e4t_conv3x3_kernel and the launch log of e4t_conv3x3 disagree, over every conv item of the corpus and conv_geometry_corpus()"""
    n = bad = 0
    syms = collections.Counter()
    for item in itertools.chain(corpus(), conv_geometry_corpus()):
        if item.kind != "conv":
            continue
        d = make_desc(item)
        said = dumper.conv_kernel(item, d)
        rc, err, lines = dumper.launch(item, d)
        if lines:
            m = re.match(r"([^|]+)\|conv .* splitk(\d+)\|", lines[0])
            ran = "%s splitk%s" % m.groups() if m else lines[0]
        else:
            ran = "rc %d %s" % (rc, err)
        n += 1
        syms[said.split(" splitk")[0] if lines else "(refused)"] += 1
        if said != ran:
            bad += 1
            print("DIFF conv %s: query %s, launch %s" % (describe(item.kw), said, ran))
    for sym, k in sorted(syms.items()):
        print("%8d  %s" % (k, sym))
    print("conv: %d rows, %d differ" % (n, bad))
    return bad


def gemm_check(dumper):
    """rows on which e4t_gemm_kernel / e4t_gemm_tn_kernel and the launch log of e4t_gemm_nt / e4t_gemm_tn disagree, over every gemm and tn item of
    the corpus.  The log carries the symbol, the split-K and the reduce kernel; store path, tail rows and colstats come from the same function
    (gemm.hip: decide_launch / resolve_tn) and are counted here per (symbol, store path)."""
    n = bad = refused = 0
    seen = collections.Counter()
    for item in corpus():
        if item.kind not in ("gemm", "tn"):
            continue
        d = make_desc(item)
        said = dumper.gemm_kernel(item, d)
        rc, err, lines = dumper.launch(item, d)
        if lines:
            m = re.match(r"([^|]+)\|gemm\w* .* splitk(\d+) flags\d+\|", lines[0])
            ran = ["%s splitk%s" % m.groups()] if m else [lines[0]]
            ran += [l.split("|")[0] for l in lines[1:]]
            f = said.split(" ") if not said.startswith("rc ") else [said]
            i = next((j for j, w in enumerate(f) if w.startswith("splitk") and w[6:].isdigit()), 0)
            got = [" ".join(f[:i + 1])] + [w for w in f[i + 2:] if w.startswith("splitk_reduce")]
            seen[" ".join(f[:i]) + " | " + (f[i + 1] if len(f) > i + 1 else "?")] += 1
        else:
            ran, got = ["rc %d %s" % (rc, err)], [said]
            refused += got == ran
        n += 1
        if got != ran:
            bad += 1
            print("DIFF %s %s: query %s, launch %s" % (item.kind, describe(item.kw), said, ran))
    for sym, k in sorted(seen.items()):
        print("%8d  %s" % (k, sym))
    print("gemm: %d rows (%d refused alike), %d differ; %d (symbol, store path) pairs" % (n, refused, bad, len(seen)))
    return bad


def attn_launch_lines(dumper):
    """the 'attn' group as the launch log tells it: descriptor -> forward | dQ | dK/dV symbol | the workspace floats the library asks for"""
    for item in attn_corpus():
        _, _, lines = dumper.attn_launch(item.kw)
        full = dumper.lib.e4t_attention_bwd_workspace_floats(*[item.kw[k] for k in ("B", "H", "T", "S", "DH")])
        yield "attn %s -> %s | %d" % (describe(item.kw), " | ".join(l.split("|")[0] for l in lines), full)


def attn_check(dumper, path):
    """rows of an --attn-launches dump that e4t_attention_plan of this library does not reproduce: the three symbols, the workspace floats and, where
    the full workspace is offered, a tsplit that explains them (total = Delta + 4 + tsplit * B * H * 2 * S * DH, or 3 * Delta + 4 un-split)"""
    want = dict(l.rstrip("\n").split(" -> ") for l in open(path) if l.startswith("attn "))
    bad = 0
    for item in attn_corpus():
        desc, kw = "attn " + describe(item.kw), item.kw
        fwd, dq, dkv, split, total = dumper.attn_plan(kw).split(" | ")
        tsplit, delta, per = int(split.split()[0]), kw["B"] * kw["H"] * kw["T"], kw["B"] * kw["H"] * 2 * kw["S"] * kw["DH"]
        fits = {1} if int(total) == 3 * delta + 4 else set()
        if (int(total) - delta - 4) % per == 0 and (int(total) - delta - 4) // per > 1:
            fits.add((int(total) - delta - 4) // per)
        if want.get(desc) != " | ".join((fwd, dq, dkv, total)) or (kw["ws"] == "full" and tsplit not in fits):
            bad += 1
            print("DIFF %s: launch log %s, plan %s" % (desc, want.get(desc), dumper.attn_plan(kw)))
    print("attn: %d rows, %d differ" % (len(want), bad))
    return bad


def write_record(dumper, path):
    if not dumper.log:      # (before the file is opened: a refused --record leaves the committed record as it is)
        sys.exit("--record needs the launch half (a machine without a GPU) to anchor the step shapes")
    digests, _ = plan_digests(dumper)
    matched, miss = anchor(dumper)
    if miss:
        sys.exit("--record: %d rows of the step table are not reproduced" % miss)
    for shape, syms in attn_step_shapes().items():      # every attention kernel the step table saw for a shape is one the plan names
        planned = dumper.attn_plan(dict(zip(("B", "H", "T", "S", "DH", "causal"), shape), ws="full")).split(" | ")[:3]
        if not set(syms) <= set(planned):
            sys.exit("--record: the step table has %s for attention %s, the plan %s" % (syms, shape, planned))
    with open(path, "w") as f:
        f.write("# What the DEFAULT build of the library plans for the corpus of tools/gemm_dispatch_dump.py (tests/test_gemm_dispatch.py).\n")
        f.write("# Regenerate after an intentional planner change: python tools/gemm_dispatch_dump.py --record\n")
        for g, (n, hx) in digests.items():
            if g != "step":
                f.write("group %s | %d | %s\n" % (g, n, hx))
        f.write("# the training step's shapes (profiles/r06_roofline_per_shape.csv), with the field combination that reproduces the recorded launch\n")
        for sym, shape, item in matched:
            f.write("step %s|%s | %s %s -> %s\n" % (sym, shape, item.kind, describe(item.kw), dumper.plan(item)))
        f.write("# the step's attention shapes (same table): forward | dQ | dK/dV kernel | tsplit tchunk | workspace floats.  Group attn was first recorded\n")
        f.write("# after --attn-check against the launch log of b388eee, the last commit before e4t_attention_plan, came out empty.\n")
        for item in attn_items(attn_step_shapes()):
            if item.kw["ws"] == "full":
                f.write("%s %s -> %s\n" % (item.kind, describe(item.kw), dumper.plan(item)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--plans", action="store_true")
    ap.add_argument("--group", action="append")
    ap.add_argument("--anchor", action="store_true")
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--conv-check", action="store_true")
    ap.add_argument("--gemm-check", action="store_true")
    ap.add_argument("--attn-launches", action="store_true")
    ap.add_argument("--attn-check", metavar="FILE")
    args = ap.parse_args()
    lib = load_lib()
    launches = not args.plans
    if launches and gpu_visible(lib):
        print("# a GPU is visible: the launch half would hand fake pointers to a real device — plan half only", flush=True)
        launches = False
    d = Dumper(launches)
    try:
        if args.record:
            write_record(d, RECORD)
            print("wrote", RECORD)
            return 0
        if args.anchor:
            if not d.log:
                sys.exit("--anchor needs the launch half")
            return 1 if anchor(d)[1] else 0
        if args.conv_check:
            if not d.log:
                sys.exit("--conv-check needs the launch half")
            return 1 if conv_check(d) else 0
        if args.gemm_check:
            if not d.log:
                sys.exit("--gemm-check needs the launch half")
            return 1 if gemm_check(d) else 0
        if args.attn_launches:
            if not d.log:
                sys.exit("--attn-launches needs the launch half")
            print("\n".join(attn_launch_lines(d)))
            return 0
        if args.attn_check:
            return 1 if attn_check(d, args.attn_check) else 0
        for item in corpus():
            if args.group and item.group not in args.group:
                continue
            print(d.line(item))
        return 0
    finally:
        d.close()


if __name__ == "__main__":
    sys.exit(main())
