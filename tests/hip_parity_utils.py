"""Helpers shared by the -m gpu parity tests: HIP product path vs the CPU oracle / golden vectors."""
import math

import numpy as np
import pytest
import torch

MASK32 = 0xFFFFFFFF

# The per-kernel float64 tests (tests/test_hip_seq_kernels.py, tests/test_hip_cls_reg_kernels.py; conventions in the former's
# docstring).  U: the unit roundoff of fp32.
U = 2.0 ** -24
TINY = 2.0 ** -126
NAN = float("nan")
GUARD = 256                  # sentinels after every output
SENT = -7777.0
ERR_ARG, ERR_UNSUPPORTED = -1, -3        # include/vunet_hip.h
EXP_U, LOG_U, TANH_U, SQRT_U, DIV_U, SIG_U = 6 * U, 6 * U, 10 * U, 6 * U, 5 * U, 12 * U


def hash_u32(x: np.ndarray) -> np.ndarray:
    """Bit-for-bit restatement of vunet_hash_u32 (csrc/common.h)."""
    x = x.astype(np.uint64) & MASK32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & MASK32
    x ^= x >> 15
    x = (x * 0x846CA68B) & MASK32
    x ^= x >> 16
    return x


def dropout_keep_mask(shape, p: float, seed: int) -> torch.Tensor:
    """CPU restatement of the conv prologue's keep-mask: keep iff hash(idx + seed) >= p * 2^32."""
    n = int(np.prod(shape))
    if p <= 0:
        return torch.ones(shape)
    thresh = min(int(p * 4294967296.0), 0xFFFFFFFF) or 1
    idx = (np.arange(n, dtype=np.uint64) + (seed & MASK32)) & MASK32
    keep = hash_u32(idx) >= thresh
    return torch.from_numpy(keep.astype(np.float32)).reshape(shape)


def assert_close(actual, expected, rtol=1e-4, atol=1e-4, name=""):
    a = actual.detach().float().cpu().numpy() if isinstance(actual, torch.Tensor) else np.asarray(actual)
    e = expected.detach().float().cpu().numpy() if isinstance(expected, torch.Tensor) else np.asarray(expected)
    assert a.shape == e.shape, f"{name}: shape {a.shape} vs {e.shape}"
    err = np.abs(a - e)
    tol = atol + rtol * np.abs(e)
    if not (err <= tol).all():
        i = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError(f"{name}: max abs err {err.max():.3e} (at {i}: {a[i]} vs {e[i]}), "
                             f"{(err > tol).mean() * 100:.3f}% outside rtol={rtol} atol={atol}")


def run_wgrad(ops, x1, x2, dy, k, stride, pad, in_act, drop, seed, flags):
    """One weight gradient through the C ABI: ask the library for the kernel's name and the slab count, launch
    vunet_conv2d_wgrad into NaN-filled slabs, reduce them with vunet_weightnorm_bwd (kind 1: plain dW) -> (dw, db, name).
    The tensor maxima are handed over for flags == 2 (the fp16 scheme) only."""
    import ctypes
    n, c1, hs, ws = x1.shape
    c2 = 0 if x2 is None else x2.shape[1]
    cout, ho, wo = dy.shape[1:]
    ctot, ktot = c1 + c2, k * k * (c1 + c2)
    wd = ops.WgradDesc(N=n, C1=c1, C2=c2, Hs=hs, Ws=ws, Cout=cout, Ho=ho, Wo=wo, KH=k, KW=k, stride=stride, pad=pad,
                       in_act=in_act, in_slope=0.0, drop_p=drop, drop_seed=seed, nsplit=1, flags=flags)
    buf = ctypes.create_string_buffer(96)
    ops._call("vunet_conv2d_wgrad_variant", ctypes.byref(wd), buf, 96)
    ns = ops._lib.lib().vunet_conv2d_wgrad_nsplit(ctypes.byref(wd))
    assert ns >= 1
    wd.nsplit = ns
    cp = ops._r32(cout)
    slabs = torch.full((ns * cp * ktot + ns * cp,), float("nan"), device="cuda")
    dshift = slabs[ns * cp * ktot:]
    amx = ops.absmax_partials(x1, x2) if flags == 2 else None
    amd = ops.absmax_partials(dy) if flags == 2 else None
    ops._call("vunet_conv2d_wgrad", ctypes.byref(wd), ops._p(x1), ops._p(x2), ops._p(dy), ops._p(slabs),
              ops._p(dshift), ops._p(amx), ops._p(amd), ops._stream())
    dw = torch.empty(cout, ctot, k, k, device="cuda")
    db = torch.empty(cout, device="cuda")
    v = torch.zeros(cout, ctot, k, k, device="cuda")
    work = torch.empty(cout * (ktot + 1), device="cuda")
    wn = ops.WnDesc(cout, c1, c2, k, k, 1, 0)
    ops._call("vunet_weightnorm_bwd", ctypes.byref(wn), ops._p(slabs), ops._p(dshift), ns, ops._p(v), None, None,
              None, None, ops._p(dw), None, ops._p(db), None, None, ops._p(work), 0, ops._stream())
    torch.cuda.synchronize()
    return dw, db, buf.value.decode()


def wgrad_ref_fp64(ops, x1, x2, dy, k, stride, pad, in_act, drop, seed):
    """float64 reference of run_wgrad on the CPU: the prologue (ELU, the dropout keep-mask of each source), then autograd of
    conv2d with respect to the weight -> (dW, db = dy summed per channel)."""
    import torch.nn.functional as F
    xs = []
    for i, x in enumerate((x1, x2)):
        if x is None:
            continue
        t = x.double().cpu()
        if in_act == ops.ACT_ELU:
            t = F.elu(t)
        if drop > 0:
            s = seed if i == 0 else (seed + ops.SEED2_OFFSET) & 0xFFFFFFFF
            t = t * dropout_keep_mask(tuple(x.shape), drop, s).double() * float(torch.tensor(1.0 / (1.0 - drop),
                                                                                             dtype=torch.float32))
        xs.append(t)
    xin = torch.cat(xs, dim=1)
    wz = torch.zeros(dy.shape[1], xin.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    (F.conv2d(xin, wz, stride=stride, padding=pad) * dy.double().cpu()).sum().backward()
    return wz.grad, dy.double().cpu().sum(dim=(0, 2, 3))


def psnr(a: torch.Tensor, b: torch.Tensor, peak: float = 2.0) -> float:
    mse = float(((a.double().cpu() - b.double().cpu()) ** 2).mean())
    return float("inf") if mse == 0 else 10.0 * np.log10(peak * peak / mse)


def assert_ulps(got, ref, bound, name="", aten=None):
    """|got - ref| <= bound elementwise where ref is finite; where ``aten`` (ATen's fp32 result) or ref is NaN / inf, got
    must be NaN / the same inf."""
    got = got.detach().cpu().double().reshape(-1)
    ref = ref.double().reshape(-1)
    pattern = (aten.double().reshape(-1) if aten is not None else ref)
    nan = torch.isnan(pattern)
    assert torch.equal(torch.isnan(got), nan), f"{name}: NaN pattern differs at {torch.nonzero(torch.isnan(got) != nan)[:8].tolist()}"
    inf = torch.isinf(pattern)
    assert torch.equal(got[inf], pattern[inf]), f"{name}: inf pattern differs"
    fin = torch.isfinite(pattern) & torch.isfinite(ref)
    assert torch.isfinite(got[fin]).all(), f"{name}: non-finite where the reference is finite"
    b = bound.double().reshape(-1) if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
    err = (got[fin] - ref[fin]).abs()
    over = err > b[fin]
    if over.any():
        i = int(torch.nonzero(over)[0])
        raise AssertionError(f"{name}: {int(over.sum())} elements over the bound; first: got {float(got[fin][i])!r} ref "
                             f"{float(ref[fin][i])!r} err {float(err[i]):.3e} bound {float(b[fin][i]):.3e}")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def assert_same(a, b, name=""):
    """Bit for bit (NaN equal to NaN of the same bits, -0 different from +0)."""
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, f"{name}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    if not torch.equal(a, b):
        bad = torch.nonzero(a != b)
        raise AssertionError(f"{name}: {bad.shape[0]} elements differ; first at {bad[0].tolist()}")


_KEEP = []      # device copies of inputs stay referenced until the launches that read them have run (Outs.check)


def _d(t):
    if t is None:
        return None
    t = t if t.is_cuda else t.cuda()
    _KEEP.append(t)
    return t


class Outs:
    """Output buffers: NaN-filled (or pre-loaded), each followed by GUARD sentinels that ``check`` wants untouched."""

    def __init__(self):
        self.bufs = []

    def new(self, *shape, fill=NAN, dtype=torch.float32):
        n = int(math.prod(shape))
        flat = torch.empty(n + GUARD, dtype=dtype, device="cuda")
        if fill is not None:
            flat[:n] = fill
        flat[n:] = SENT
        self.bufs.append((flat, n))
        return flat[:n].view(*shape)

    def load(self, t):
        out = self.new(*t.shape, fill=None, dtype=t.dtype)
        out.copy_(t)
        return out

    def check(self):
        torch.cuda.synchronize()
        for k, (flat, n) in enumerate(self.bufs):
            assert bool((flat[n:] == SENT).all()), f"guard band of output {k} ({n} elements) was written"
        _KEEP.clear()


def _refused(ops, code, name, *args):
    with pytest.raises(RuntimeError, match=rf"{name} failed with code {code}$"):
        ops._call(name, *args)


def _adam_hp(T, lr, step, b1, b2, eps, wd, resolved=True):
    lr_dev = torch.tensor([lr], dtype=torch.float64, device="cuda")
    step_dev = torch.tensor([step], dtype=torch.int64, device="cuda")
    res = torch.zeros(2, device="cuda") if resolved else None
    hp = T.SeqAdamHp(lr_dev.data_ptr(), step_dev.data_ptr(), b1, b2, eps, wd, None if res is None else res.data_ptr())
    return hp, (lr_dev, step_dev, res)


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _adam64(p, g, m, v, step_size, inv_sqrt_bc2, b1, b2, eps, wd, dg):
    """seq_adam.h's update in float64 from the fp32 state and the fp32 constants, with its bound given the gradient's (dg):
    m: (1 - b1) dg + 3 U (b1 |m| + (1 - b1) |g|); v: (1 - b2) 2 |g| dg + 4 U (b2 v + (1 - b2) g^2); denom = sqrtf(v) k + eps: v's
    error through the root + (sqrtf + 2 roundings) relative; p -= step (m / denom): the quotient's parts + (division + product +
    the difference) relative."""
    b1, b2, eps, wd = _f32(b1), _f32(b2), _f32(eps), _f32(wd)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    g = g + wd * p
    dg = dg + 2 * U * wd * p.abs()
    m2 = b1 * m + (1 - b1) * g
    dm = (1 - b1) * dg + 3 * U * (b1 * m.abs() + (1 - b1) * g.abs())
    v2 = b2 * v + (1 - b2) * g * g
    dv = (1 - b2) * (2 * g.abs() * dg + dg * dg) + 4 * U * (b2 * v + (1 - b2) * g * g)
    root = v2.sqrt()
    droot = torch.minimum(dv / (2 * root.clamp_min(TINY)), dv.sqrt())
    denom = root * inv_sqrt_bc2 + eps
    ddenom = droot * inv_sqrt_bc2 + (SQRT_U + 2 * U) * denom
    upd = step_size * m2 / denom
    dupd = step_size * dm / denom + upd.abs() * (ddenom / denom + DIV_U + 2 * U)
    return (p - upd, dupd + U * (p.abs() + upd.abs()) + TINY), (m2, dm + TINY), (v2, dv + TINY)
