"""Build + load libvunet_hip.so (the C-ABI HIP library, include/vunet_hip.h).

The library is built in-tree with hipcc for gfx950 only and loaded with ctypes.  There is no CPU
fallback: if the shared object is missing, or no GPU is present when a kernel is requested, the
product path raises.
"""
from __future__ import annotations

import ast
import ctypes
import functools
import operator
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.path.join(PKG_DIR, "libvunet_hip.so")
INCLUDE_DIR = os.path.join(os.path.dirname(PKG_DIR), "include")
HEADER = os.path.join(INCLUDE_DIR, "vunet_hip.h")
ARCH = "gfx950"


def headers() -> list:
    """Every public header of the C ABI (include/*.h): vunet_hip.h and the per-family headers beside it."""
    return sorted(os.path.join(INCLUDE_DIR, f) for f in os.listdir(INCLUDE_DIR) if f.endswith(".h"))


def _deps_of(src: str, seen=None) -> list:
    """``src`` and the project headers it includes (transitively; ``#include "..."`` resolved beside the includer)."""
    seen = set() if seen is None else seen
    if src in seen or not os.path.isfile(src):
        return []
    seen.add(src)
    out = [src]
    for inc in re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(src).read(), flags=re.M):
        out += _deps_of(os.path.normpath(os.path.join(os.path.dirname(src), inc)), seen)
    return out


def _sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = _sources() + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + headers()
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 every csrc/*.hip and link libvunet_hip.so (cross-compiles without a GPU)."""
    if not force and not _needs_build():
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(PKG_DIR, "build")
    os.makedirs(objdir, exist_ok=True)
    flags = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        deps = _deps_of(src)   # the source and the headers it actually includes: a new entry point rebuilds its own file only
        if not force and os.path.exists(obj) and all(os.path.getmtime(obj) >= os.path.getmtime(d) for d in deps):
            return obj
        cmd = [hipcc] + flags + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr}")
        return obj

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, _sources()))
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB_PATH] + objs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stderr}")
    return LIB_PATH


@functools.lru_cache(maxsize=None)
def _header_text() -> str:
    """include/*.h in one string, comments stripped (read once: the headers do not change under a running process)."""
    txt = "\n".join(open(h).read() for h in headers())
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def declared_symbols() -> list:
    """Function names declared in include/*.h."""
    txt = _header_text()
    return sorted(set(re.findall(r"\bint\s+(vunet_[a-z0-9_]+)\s*\(", txt)))


_CTYPE = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
          "float": ctypes.c_float, "double": ctypes.c_double, "int": ctypes.c_int}


def declared_prototypes() -> dict:
    """name -> list of ctypes argument types, parsed from include/*.h (single source of truth)."""
    txt = _header_text()
    protos = {}
    for m in re.finditer(r"\bint\s+(vunet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt, flags=re.S):
        name, args = m.group(1), m.group(2).strip()
        types = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                if "*" in a:
                    types.append(ctypes.c_void_p)
                else:
                    types.append(_CTYPE[a.replace("const ", "").split(" ")[0]])
        protos[name] = types
    return protos


# ---- descriptor structs and integer constants come from the same headers: Python holds no second copy of either
def _members(cname: str, decl: str, structs: dict) -> list:
    """The (name, ctype) fields of one member declaration (whitespace normalised) of struct ``cname``."""
    dm = re.fullmatch(r"(?:const )?(\w+)\b ?(.+)", decl)
    base, fields = dm.group(1) if dm else None, []
    ctype = _CTYPE.get(base) or structs.get(base)
    for part in dm.group(2).split(",") if dm else [""]:
        pm = re.fullmatch(r"(\*?) ?([A-Za-z_]\w*)", part.strip())
        if pm is None or (ctype is None and not (pm.group(1) and base == "void")):
            raise ValueError(f"struct {cname}: unsupported declaration `{decl};`")
        fields.append((pm.group(2), ctypes.c_void_p if pm.group(1) else ctype))
    return fields


def parse_structs(txt: str) -> dict:
    """cname -> ctypes.Structure subclass for every ``typedef struct [tag] { ... } cname;`` of the comment-stripped header text,
    in order.  A member is ``[const] T a, b;`` or ``[const] T *a, *b;``, T a fixed-width scalar, ``void`` (pointers only) or a struct
    declared earlier; a pointer is a ``c_void_p``.  Anything else (an unknown type, a bitfield, an array, a union, a function
    pointer) raises ValueError with the struct and the declaration: nothing is skipped."""
    structs = {}
    for m in re.finditer(r"\btypedef\s+struct\b\s*(\w*)\s*\{", txt):
        end = txt.find("}", m.end())
        tail = re.match(r"\}\s*(\w+)\s*;", txt[end:]) if end >= 0 else None
        body = txt[m.end():end]
        if tail is None or "{" in body:
            raise ValueError(f"struct {m.group(1)}: braces inside the body (a union, an inner struct) or no closing `}} name;`")
        cname = tail.group(1)
        fields = [f for decl in body.split(";") if decl.strip() for f in _members(cname, " ".join(decl.split()), structs)]
        structs[cname] = type(cname, (ctypes.Structure,), {"_fields_": fields})
    return structs


_TOKEN = r"0[xX][0-9a-fA-F]+|[1-9][0-9]*|0|[A-Za-z_]\w*|<<|[-+*()]"
_BINOP = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul, ast.LShift: operator.lshift}
_FLOAT = r"[-+]?((\d+\.\d*|\.\d+)([eE][-+]?\d+)?|\d+[eE][-+]?\d+)[fFlL]?"


def _eval_int(body: str, known: dict) -> int:
    """A macro body of decimal / hex literals, names in ``known`` and ``+ - * << ( )`` (C and Python agree on their precedence)."""
    def ev(n):
        if isinstance(n, ast.Constant):
            return n.value
        if isinstance(n, ast.Name) and n.id in known:
            return known[n.id]
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, (ast.USub, ast.UAdd)):
            return -ev(n.operand) if isinstance(n.op, ast.USub) else ev(n.operand)
        if isinstance(n, ast.BinOp) and type(n.op) in _BINOP:
            return _BINOP[type(n.op)](ev(n.left), ev(n.right))
        raise ValueError(ast.dump(n))
    if not re.fullmatch(rf"(\s*({_TOKEN}))+\s*", body):
        raise ValueError("a character outside the grammar")
    return ev(ast.parse(" ".join(re.findall(_TOKEN, body)), mode="eval").body)   # (tokens re-joined: no Python-only spelling gets in)


def parse_constants(txt: str) -> dict:
    """name -> int for the object-like ``#define VUNET_*`` macros of the comment-stripped header text.  No constants, by rule:
    macros of another namespace, function-like macros, empty bodies (the include guards) and a body that is one floating-point
    literal.  Every other body must be an integer expression of literals and EARLIER macros (``_eval_int``), or this raises."""
    consts = {}
    for name, params, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(\(?)(.*)$", txt, flags=re.M):
        body = body.strip()
        if name.startswith("VUNET_") and not params and body and not re.fullmatch(_FLOAT, body):
            try:
                consts[name] = _eval_int(body, consts)
            except (ValueError, SyntaxError) as e:
                raise ValueError(f"#define {name} {body}: not an integer expression ({e})") from None
    return consts


@functools.lru_cache(maxsize=None)
def structs() -> dict:
    """cname -> ctypes.Structure subclass for every struct of include/*.h (parsed once; the dict is shared: read it only)."""
    return parse_structs(_header_text())


@functools.lru_cache(maxsize=None)
def constants() -> dict:
    """name -> value of every integer ``#define VUNET_*`` of include/*.h (parsed once; the dict is shared: read it only)."""
    return parse_constants(_header_text())


def struct(cname: str):
    """The class of ``typedef struct ... cname;``.  Bind it at import, as ``const``'s values: no launch path looks either up."""
    return structs()[cname]


def const(name: str) -> int:
    return constants()[name]


_LIB = None


def lib() -> ctypes.CDLL:
    """The loaded library.  Raises if it has not been built -- there is no fallback."""
    global _LIB
    if _LIB is None:
        # PyTorch ships its own libamdhip64: it must be the HIP runtime this library binds to (same
        # streams / allocations), so torch is imported -- and its runtime loaded -- before the dlopen.
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the HIP extension is mandatory, there is no CPU fallback)")
        # VUNET_HIP_LIB: an alternative build of the same library (kernel tuning A/B runs: tools/ab_build.sh)
        _LIB = ctypes.CDLL(os.environ.get("VUNET_HIP_LIB", LIB_PATH))
        for name, argtypes in declared_prototypes().items():
            fn = getattr(_LIB, name)  # AttributeError if the .so is stale
            fn.restype = ctypes.c_int
            fn.argtypes = argtypes
    return _LIB
