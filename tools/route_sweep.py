"""Which kernel does every convolution problem get?  Host logic only, no GPU.

    python tools/route_sweep.py compare <lib-a.so> <lib-b.so>     # every sweep on both libraries, byte for byte
    python tools/route_sweep.py table <lib.so> <commit> > tests/route_table.txt
    python tools/route_sweep.py sweep --side conv --grid thin --out lines.txt   # one sweep of $VUNET_HIP_LIB, as text

A sweep enumerates descriptors (GRIDS) and writes one line per case: the descriptor, then what the query entry points
answer for it (conv side: vunet_conv2d_x6_supported, vunet_conv2d_gather_variant, and per scheme 0 / 1 / 2
vunet_conv2d_variant, vunet_conv2d_publishes_amax, vunet_conv2d_wants_split; wgrad side: vunet_conv2d_wgrad_variant,
_nsplit, _wants_split, _batchable), return codes included.  `compare` runs the full grid with the default settings and
the thin grid once per tuning key / environment flag the routers read (SETTINGS; each in a process of its own: the
library reads the environment once), on both libraries, compares the SHA-256 of every output and prints how many
cases reached each kernel family; it fails if the outputs differ or if a family is never reached on <lib-a>.
`table` samples the full default sweep of one library evenly per family into a table a test can replay (replay()).
"""
import argparse
import ctypes
import hashlib
import itertools
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CH = (3, 4, 8, 16, 32, 48, 64, 128, 256, 512)
MAPS = tuple((s, s) for s in (4, 8, 16, 32, 64, 128, 256)) + ((16, 24), (12, 32), (8, 16))
# (in_act, drop_p): the four prologue codes -- none, ELU, ELU + dropout, generic
PROLOGUES = ((0, 0.0), (1, 0.0), (1, 0.1), (4, 0.0))
GRIDS = {
    "full": dict(N=(1, 2, 16), C=CH, M=CH, maps=MAPS),
    "thin": dict(N=(2, 16), C=(3, 16, 64, 128), M=(3, 16, 64, 128), maps=((8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (16, 24))),
}
TUNE = {"split_force_nt": 0, "tiled_force_nt": 1, "force_small": 2, "parity_launches": 4, "wgrad_rowsplit": 6, "s2_fwd_f32": 7}
# (side, tuning key or environment variable, value)
SETTINGS = ([("conv", "split_force_nt", v) for v in (1, 2, 4)] + [("conv", "tiled_force_nt", v) for v in (1, 2, 4)] +
            [("conv", "force_small", 1), ("conv", "parity_launches", 1), ("conv", "s2_fwd_f32", 1)] +
            [("wgrad", "wgrad_rowsplit", v) for v in (1, 2, 3, 4)] +
            [("conv", "VUNET_NO_TILED", "1"), ("conv", "VUNET_NO_PHASE", "1"), ("conv", "VUNET_NO_1X1", "1"),
             ("conv", "VUNET_NO_THIN", "1"), ("conv", "VUNET_NO_THIN_KV", "1"), ("conv", "VUNET_CONV_PRECISION", "f32"),
             ("wgrad", "VUNET_CONV_PRECISION", "f32"), ("wgrad", "VUNET_WGRAD_BATCH_PIX", "4096"),
             ("wgrad", "VUNET_WGRAD_SPLIT_WGS", "256")])
CONV_FAMILIES = ("phase", "thin", "1x1", "tiled", "gather", "splitk", "h2_s2", "h2_small", "h2_w16", "h2_parity", "h2", "x6",
                 "unsupported")
WGRAD_FAMILIES = ("x6", "h2", "direct", "thin", "tiled", "generic")
CONV_KEYS = ("N", "C1", "C2", "Hs", "Ws", "M", "m_off", "Mpad", "Ho", "Wo", "KH", "KW", "stride", "pad", "mode", "in_act",
             "drop_p", "d2s")
WGRAD_KEYS = ("N", "C1", "C2", "Hs", "Ws", "Cout", "Ho", "Wo", "KH", "KW", "stride", "pad", "in_act", "drop_p", "flags")


def conv_family(name):
    if name.startswith("conv_gather_kernel<phase"): return "phase"
    if name.startswith("conv_h2_kernel"):
        if name.endswith(", 16>"): return "h2_w16"
        return "h2_parity" if "parity" in name or name.endswith("<1, 1, 1, 0, 4, 4, 32>") else "h2"
    for prefix, fam in (("conv_thin_", "thin"), ("conv_1x1_", "1x1"), ("conv_tiled_", "tiled"), ("conv_gather_splitk", "splitk"),
                        ("conv_gather_kernel", "gather"), ("conv_h2_s2_", "h2_s2"), ("conv_h2_small_", "h2_small"),
                        ("conv_x6_", "x6")):
        if name.startswith(prefix): return fam
    return "unsupported"


def wgrad_family(name):
    for prefix, fam in (("conv_wgrad_x6_", "x6"), ("conv_wgrad_h2_", "h2"), ("conv_wgrad_direct_", "direct"),
                        ("conv_wgrad_s2_", "direct"), ("conv_wgrad_thin_", "thin"), ("conv_wgrad_tiled_", "tiled")):
        if name.startswith(prefix): return fam
    return "generic"


def conv_cases(grid):
    """(descriptor fields, has_aux, has_res, has_mask): the grid, fully crossed."""
    g = GRIDS[grid]
    for N, C1, two, M, (H, W), K, s, mode in itertools.product(g["N"], g["C"], (0, 1), g["M"], g["maps"], (1, 3, 4), (1, 2), (0, 1)):
        pad = 0 if K == 1 else 1
        if mode == 0: Ho, Wo = (H + 2 * pad - K) // s + 1, (W + 2 * pad - K) // s + 1
        elif s == 2: Ho, Wo = 2 * H, 2 * W            # transposed gather over the dy map: the stride-2 layer's input
        else: Ho, Wo = H + K - 1 - 2 * pad, W + K - 1 - 2 * pad
        if Ho < 1 or Wo < 1: continue
        for (act, drop), d2s, m_off in itertools.product(PROLOGUES, (0, 1), (0, 32)):
            d = dict(N=N, C1=C1, C2=C1 if two else 0, Hs=H, Ws=W, M=M, m_off=m_off, Mpad=(m_off + M + 31) // 32 * 32, Ho=Ho,
                     Wo=Wo, KH=K, KW=K, stride=s, pad=pad, mode=mode, in_act=act, drop_p=drop, d2s=d2s)
            for flags in itertools.product((0, 1), repeat=3):
                yield (d,) + flags


def wgrad_cases(grid):
    g = GRIDS[grid]
    for N, C1, two, M, (H, W), K, s, (act, drop), flags in itertools.product(g["N"], g["C"], (0, 1), g["M"], g["maps"], (1, 3, 4),
                                                                          (1, 2), PROLOGUES, (0, 1, 2, 3)):
        pad = 0 if K == 1 else 1
        Ho, Wo = (H + 2 * pad - K) // s + 1, (W + 2 * pad - K) // s + 1
        if Ho < 1 or Wo < 1: continue
        yield dict(N=N, C1=C1, C2=C1 if two else 0, Hs=H, Ws=W, Cout=M, Ho=Ho, Wo=Wo, KH=K, KW=K, stride=s, pad=pad, in_act=act,
                   drop_p=drop, flags=flags)


class Queries:
    """The query entry points of one loaded library, answering in the text of a sweep line."""

    def __init__(self):
        from behavior_driven_video_synthesis_amd import _lib, ops
        self.lib, self.ops = _lib.lib(), ops
        self.buf = ctypes.create_string_buffer(128)

    def _named(self, rc):
        return f"{rc}:{self.buf.value.decode()}" if rc == 0 else f"{rc}:"

    def conv(self, d, aux, res, mask):
        """-> (result text, family per scheme, x6_supported)"""
        L, buf = self.lib, self.buf
        p = ctypes.byref(self.ops.ConvDesc(in_slope=0.2, drop_seed=7, out_act=0, **d))
        sup = L.vunet_conv2d_x6_supported(p, mask)
        out = [str(sup), self._named(L.vunet_conv2d_gather_variant(p, aux, buf, 128))]
        fams = []
        for scheme in (0, 1, 2):
            rc = L.vunet_conv2d_variant(p, aux, scheme, mask, buf, 128)
            fams.append(conv_family(buf.value.decode()) if rc == 0 else "unsupported")
            out.append(f"{self._named(rc)} {L.vunet_conv2d_publishes_amax(p, aux, res, scheme)}"
                       f" {L.vunet_conv2d_wants_split(p, aux, res, mask, scheme)}")
        return "|".join(out), fams, sup

    def wgrad(self, d):
        L = self.lib
        p = ctypes.byref(self.ops.WgradDesc(in_slope=0.2, drop_seed=7, nsplit=1, **d))
        rc = L.vunet_conv2d_wgrad_variant(p, self.buf, 128)
        fam = wgrad_family(self.buf.value.decode())
        return (f"{self._named(rc)}|{L.vunet_conv2d_wgrad_nsplit(p)}|{L.vunet_conv2d_wgrad_wants_split(p)}"
                f"|{L.vunet_conv2d_wgrad_batchable(p)}"), fam


def conv_line(q, d, aux, res, mask):
    text, fams, sup = q.conv(d, aux, res, mask)
    return f"c {' '.join(str(d[k]) for k in CONV_KEYS)} {aux} {res} {mask}|{text}", fams, sup


def wgrad_line(q, d):
    text, fam = q.wgrad(d)
    return f"w {' '.join(str(d[k]) for k in WGRAD_KEYS)}|{text}", fam


def replay(q, line):
    """Recompute a sweep line's answers from its descriptor on the loaded library -> the line as it comes out now."""
    f = line.split("|", 1)[0].split()
    num = [float(x) if "." in x else int(x) for x in f[1:]]
    if f[0] == "c":
        return conv_line(q, dict(zip(CONV_KEYS, num)), *num[len(CONV_KEYS):])[0]
    return wgrad_line(q, dict(zip(WGRAD_KEYS, num)))[0]


class Sampler:
    """Keeps at most `cap` lines per family, evenly spread over the order they arrive in (deterministic)."""

    def __init__(self, cap):
        self.cap, self.kept, self.seen, self.stride = cap, {}, {}, {}

    def add(self, fam, line):
        n = self.seen[fam] = self.seen.get(fam, -1) + 1
        st = self.stride.setdefault(fam, 1)
        if n % st: return
        k = self.kept.setdefault(fam, [])
        k.append(line)
        if len(k) > self.cap:
            self.kept[fam], self.stride[fam] = k[::2], st * 2


def sweep(a):
    for kv in a.tune:
        k, v = kv.split("=")
        from behavior_driven_video_synthesis_amd import ops
        ops.set_tuning(k, int(v))
    q, sha, count, n = Queries(), hashlib.sha256(), {}, 0
    out = open(a.out, "w") if a.out else None
    sampler = Sampler(a.sample) if a.sample else None
    cases = conv_cases(a.grid) if a.side == "conv" else wgrad_cases(a.grid)
    for case in itertools.islice(cases, a.shard, None, a.shards):
        if a.side == "conv":
            line, fams, sup = conv_line(q, *case)
            keys = [f"s{s}:{fam}" for s, fam in enumerate(fams)] + ([] if sup else ["x6:unsupported"])
        else:
            line, fam = wgrad_line(q, case)
            keys = [fam]
        for k in keys: count[k] = count.get(k, 0) + 1
        if sampler:
            for k in set(keys): sampler.add(k, line)
        sha.update(line.encode() + b"\n")
        if out: out.write(line + "\n")
        n += 1
    print(json.dumps(dict(cases=n, sha256=sha.hexdigest(), families=count, sample=sampler.kept if sampler else None)))


def run(lib, side, grid, setting=None, shards=8, sample=0):
    """One sweep of `lib` in `shards` child processes -> (digests, family counts, samples)."""
    env = dict(os.environ, VUNET_HIP_LIB=os.path.abspath(lib))
    cmd = [sys.executable, os.path.abspath(__file__), "sweep", "--side", side, "--grid", grid, "--shards", str(shards),
           "--sample", str(sample)]
    if setting and setting[0] in TUNE: cmd += ["--tune", f"{setting[0]}={setting[1]}"]
    elif setting: env[setting[0]] = str(setting[1])
    with ThreadPoolExecutor(max_workers=shards) as ex:
        res = list(ex.map(lambda i: json.loads(subprocess.run(cmd + ["--shard", str(i)], env=env, check=True,
                                                              capture_output=True, text=True).stdout), range(shards)))
    fam = {}
    for r in res:
        for k, v in r["families"].items(): fam[k] = fam.get(k, 0) + v
    return [r["sha256"] for r in res], sum(r["cases"] for r in res), fam, [r["sample"] for r in res]


def jobs():
    yield "conv", "full", None
    yield "wgrad", "full", None
    for side, key, val in SETTINGS: yield side, "thin", (key, val)


def missing_families(fam, side):
    if side == "wgrad": return [f for f in WGRAD_FAMILIES if not fam.get(f)]
    reached = {k.split(":")[1] for k, v in fam.items() if v}
    return [f for f in CONV_FAMILIES if f not in reached]


def compare(a):
    def one(job):
        side, grid, setting = job
        shards = 4 if grid == "full" else 1
        return job, run(a.lib_a, side, grid, setting, shards), run(a.lib_b, side, grid, setting, shards)
    bad = 0
    with ThreadPoolExecutor(max_workers=a.jobs) as ex:
        for (side, grid, setting), ra, rb in ex.map(one, jobs()):
            same = ra[0] == rb[0] and ra[1] == rb[1]
            print(f"{side} {grid} {setting or 'defaults'}: {ra[1]} cases, {'identical' if same else 'DIFFERENT'}")
            print("   families on a:", json.dumps(ra[2], sort_keys=True))
            if not setting and missing_families(ra[2], side):
                print("   NEVER REACHED on a:", missing_families(ra[2], side))
                bad += 1
            bad += not same
    sys.exit(1 if bad else 0)


FLAGS3 = tuple(itertools.product((0, 1), repeat=3))


def pack(lines):
    """Sweep lines -> the table's text: `= <answers>` lines number the distinct answer texts, then one line per descriptor
    with the answer numbers of its cases -- conv: (has_aux, has_res, has_mask) in the order of FLAGS3, wgrad: flags 0..3."""
    answers, groups = {}, {}
    for line in lines:
        head, text = line.split("|", 1)
        f = head.split()
        cut = -3 if f[0] == "c" else -1
        groups.setdefault(" ".join(f[:cut]), {})[" ".join(f[cut:])] = answers.setdefault(text, len(answers))
    out = [f"= {t}" for t in answers]
    for desc in sorted(groups):
        order = [" ".join(map(str, fl)) for fl in FLAGS3] if desc[0] == "c" else ["0", "1", "2", "3"]
        out.append(desc + "|" + " ".join(str(groups[desc][k]) for k in order))
    return out


def unpack(rows):
    """The inverse of pack(): the table's rows (comment lines dropped) -> sweep lines."""
    answers = [r[2:] for r in rows if r.startswith("= ")]
    for r in rows:
        if r[0] in "cw":
            desc, idx = r.split("|")
            order = [" ".join(map(str, fl)) for fl in FLAGS3] if r[0] == "c" else ["0", "1", "2", "3"]
            for k, i in zip(order, idx.split()):
                yield f"{desc} {k}|{answers[int(i)]}"


def table(a):
    print(f"# routing answers recorded from commit {a.commit} by tools/route_sweep.py table (format: pack()); replayed by"
          " tests/test_cabi_and_host.py.  Never regenerate from the code under test.")
    os.environ["VUNET_HIP_LIB"] = os.path.abspath(a.lib)
    q, lines = Queries(), set()
    for side in ("conv", "wgrad"):
        _, _, fam, samples = run(a.lib, side, "full", None, shards=8, sample=a.cap)
        assert not missing_families(fam, side), missing_families(fam, side)
        per = {}
        for s in samples:
            for k, v in s.items(): per.setdefault(k, []).extend(v)
        for k in sorted(per):   # `cap` descriptors per family, each with all its flag cases
            v = per[k]
            for line in v[::max(1, len(v) // a.cap)][:a.cap]:
                f = line.split("|", 1)[0].split()
                if side == "conv": lines.update(replay(q, " ".join(f[:-3] + list(map(str, fl))) + "|") for fl in FLAGS3)
                else: lines.update(replay(q, " ".join(f[:-1] + [str(fl)]) + "|") for fl in range(4))
    print("\n".join(pack(sorted(lines))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("sweep")
    s.add_argument("--side", choices=("conv", "wgrad"), required=True)
    s.add_argument("--grid", choices=tuple(GRIDS), default="full")
    s.add_argument("--tune", action="append", default=[])
    s.add_argument("--shard", type=int, default=0)
    s.add_argument("--shards", type=int, default=1)
    s.add_argument("--sample", type=int, default=0)
    s.add_argument("--out")
    s.set_defaults(fn=sweep)
    c = sub.add_parser("compare")
    c.add_argument("lib_a")
    c.add_argument("lib_b")
    c.add_argument("--jobs", type=int, default=2)
    c.set_defaults(fn=compare)
    t = sub.add_parser("table")
    t.add_argument("lib")
    t.add_argument("commit")
    t.add_argument("--cap", type=int, default=30)
    t.set_defaults(fn=table)
    a = ap.parse_args()
    a.fn(a)
