"""Pin what ops.FusedConv and the deferred weight-gradient queue DO, for host-side refactors (needs the GPU).

    python tools/fused_conv_trace.py record run1.json [values]             # in a checkout of the PARENT commit, ...
    python tools/fused_conv_trace.py record run2.json                      # ... twice, in two fresh processes
    python tools/fused_conv_trace.py merge run1.json run2.json <commit> > tests/fused_conv_trace.json
    python tools/fused_conv_trace.py check tests/fused_conv_trace.json     # the tree under test against the fixture
    python tools/fused_conv_trace.py --cases=seq_host_cases record|merge|check ...   # the same for tests/seq_host_trace.json

`record` runs every case of tests/fused_conv_cases.py (copy that file and this one into the parent's checkout: they use
only what both trees have), or of another cases module under tests/ named by a leading `--cases=MODULE` (one with CASES,
record_case and missing_coverage: tests/seq_host_cases.py pins the seq engines' host code in tests/seq_host_trace.json) and writes the records and, with `values`, the tensors' bytes beside them (<out>.npz: needed
only if a hash differs between the two recordings).  `merge` refuses
recordings whose traces or profile triples differ or that miss a required entry point / return code; a tensor whose hash
differs between the two is pinned by value instead (base64 fp32 in the fixture's "loose" section, listed in its header,
compared at 1e-6 of its max-abs).  Never regenerate the fixture from the code under test.
"""
import base64
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


CASES_MODULE = "fused_conv_cases"


def record(out, values=None):
    fc = importlib.import_module(CASES_MODULE)
    records, blobs = {}, {}
    for name in fc.CASES:
        records[name], raw = fc.record_case(name)
        blobs.update({f"{name}/{k}": np.frombuffer(b, dtype=np.float32) for k, b in raw.items()})
        print(name, len(records[name]["trace"]), "calls", flush=True)
    missing = fc.missing_coverage(records)
    json.dump({"cases": records, "missing": missing}, open(out, "w"))
    if values:
        np.savez(os.path.splitext(out)[0] + ".npz", **blobs)
    print("missing coverage (merge refuses the recording if any):", missing)
    return 0


def merge(a_path, b_path, commit):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    assert not a["missing"] and not b["missing"], (a["missing"], b["missing"])
    loose = {}
    for name, ra in a["cases"].items():
        rb = b["cases"][name]
        for part in ("trace", "profile", "absent"):
            assert ra[part] == rb[part], f"{name}: {part} differs between the two recordings -- the case is ill-posed"
        for k in [k for k, h in ra["sha256"].items() if rb["sha256"][k] != h]:
            values = np.load(os.path.splitext(a_path)[0] + ".npz")   # (record ... values)
            loose.setdefault(name, {})[k] = base64.b64encode(values[f"{name}/{k}"].tobytes()).decode()
            del ra["sha256"][k]
    header = (f"recorded from commit {commit} by tools/fused_conv_trace.py; not bitwise-pinned (compared by value): "
              f"{sorted(f'{n}/{k}' for n, d in loose.items() for k in d) or 'none'}")
    rows = ",\n".join(f"{json.dumps(n)}: {json.dumps(r)}" for n, r in a["cases"].items())   # one case per line
    print(f'{{"header": {json.dumps(header)},\n"cases": {{\n{rows}\n}},\n"loose": {json.dumps(loose)}}}')
    return 0


def compare(fixture, name, rec, raw):
    """Differences between a fresh record of case ``name`` and the fixture (empty: it matches)."""
    want, bad = fixture["cases"][name], []
    if rec["trace"] != want["trace"]:
        i = next((i for i, (x, y) in enumerate(zip(rec["trace"], want["trace"])) if x != y), min(len(rec["trace"]), len(want["trace"])))
        bad.append(f"trace differs at call {i}: got {rec['trace'][i:i + 3]}, recorded {want['trace'][i:i + 3]}")
    if rec["profile"] != want["profile"]:
        bad.append(f"profile triples differ: got {rec['profile']}, recorded {want['profile']}")
    if rec["absent"] != want["absent"]:
        bad.append(f"absent tensors differ: got {rec['absent']}, recorded {want['absent']}")
    loose = fixture["loose"].get(name, {})
    if set(rec["sha256"]) != set(want["sha256"]) | set(loose):
        bad.append(f"tensor names differ: got {sorted(rec['sha256'])}")
    bad += [f"{k}: bytes differ from the recording" for k, h in want["sha256"].items() if rec["sha256"].get(k) != h]
    for k, b64 in loose.items():
        ref, got = np.frombuffer(base64.b64decode(b64), dtype=np.float32), np.frombuffer(raw[k], dtype=np.float32)
        err = float(np.abs(got - ref).max()) if got.shape == ref.shape else float("inf")
        print(f"{name}/{k}: max |difference| {err:.3e}, bound {1e-6 * float(np.abs(ref).max()):.3e}")
        if not err <= 1e-6 * float(np.abs(ref).max()):
            bad.append(f"{k}: differs from the recorded values by {err:.3e}")
    return bad


def check(path):
    fc = importlib.import_module(CASES_MODULE)
    fixture, failed = json.load(open(path)), 0
    for name in fc.CASES:
        bad = compare(fixture, name, *fc.record_case(name))
        print(name, "ok" if not bad else bad, flush=True)
        failed += bool(bad)
    return 1 if failed else 0


if __name__ == "__main__":
    cmds = {"record": record, "merge": merge, "check": check}
    if len(sys.argv) > 1 and sys.argv[1].startswith("--cases="):
        CASES_MODULE = sys.argv.pop(1)[len("--cases="):]
    if len(sys.argv) < 3 or sys.argv[1] not in cmds:
        sys.exit(__doc__)
    sys.exit(cmds[sys.argv[1]](*sys.argv[2:]))
