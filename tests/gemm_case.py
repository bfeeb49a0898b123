"""Inputs, the fp64 reference and the per-element error bound of lthm_gemm (include/lthm.h):

    C[b] = epi(alpha * A[b] . B[b]),   epi: + bias, act, + res1, + res2, cast to out_dtype

tests/test_gemm_host.py pins the reference and the bound on the CPU (every listed corruption of
the reference is rejected, a float32 CPU evaluation is accepted); tests/test_gpu_gemm.py holds
every kernel of recommendations_amd/csrc/gemm.hip to them, element by element.

Everything here is plain torch on the CPU.  Nothing is imported from recommendations_amd: the
activations restate include/lthm.h (LTHM_ACT_*): 0 none, 1 tanh-GELU and 2 QuickGELU (aux_out
receives the pre-activation), 3 / 4 multiply by GELU' / QuickGELU' of aux, 5 tanh-GELU whose
aux_out receives GELU'(x), 6 multiply by aux.

The bound (bound(), derived in DESIGN.md section 17), with u = 2^-23 and S = |A| . |B|:
  x = alpha A.B + bias   e_x = |alpha| (K + 1) u S + u |x|
       products of two bf16 values are exact in f32; an f32 sum of K terms in any order, with
       rounding or truncating adders, is within K u S of the exact sum (split-K partial sums
       included); one more u S for the multiplication by alpha, one u |x| for the bias add
  y = act(x)             e_y = L e_x + T          L: the largest |act'| on the real line
  y = x act'(aux)        e_y = |act'(aux)| e_x + |x| T + u |y|       (y = x aux: T = 0)
  + res                  e  += u |running sum|    per residual
  bf16 destination       e  += 2^-8 (|ref| + e)   (C, aux_out: half an ulp of 8 significant bits; 2^-9
                         would refuse a correctly rounded store, test_gemm_host.py shows it)
T is the one measured term: 8 x the largest |formula in float32 on the CPU - formula in float64|
over the case's own arguments (the device's exp and reciprocal are not the CPU's).
"""
import functools
import math
import zlib
from collections import namedtuple
from types import SimpleNamespace

import torch

ACT_NONE, ACT_GELU, ACT_QGELU, ACT_GELU_GRAD, ACT_QGELU_GRAD, ACT_GELU_D, ACT_MUL_AUX = range(7)
GRAD_ACTS = (ACT_GELU_GRAD, ACT_QGELU_GRAD, ACT_MUL_AUX)
AUX_OUT_ACTS = (ACT_GELU, ACT_QGELU, ACT_GELU_D)
U32 = 2.0 ** -23   # one f32 ulp (relative), the error of one truncating f32 operation
U16 = 2.0 ** -8    # bf16 keeps 8 significant bits: rounding to nearest moves a value by at most 2^-8 of it

# ka / kb: the operand is K-contiguous (A [M][K], B [N][K]) or K-strided (A [K][M], B [K][N]).
# pad_*: elements added to the minimal leading dimension (lda, ldb, ldc, ldaux, ldr1 = ldr2);
# pad_s: elements added to each batch stride; off_*: element offset of the pointer (1 makes a
# bf16 pointer 2-byte aligned only); res1 / res2 / out_dtype: None, "f32" or "bf16".
Spec = namedtuple(
    "Spec", "M N K batch ka kb pad_a pad_b pad_c pad_aux pad_r pad_s off_a off_b off_c off_bias "
            "alpha bias act res1 res2 out_dtype splits amax",
    defaults=(1, True, True, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0, False, ACT_NONE, None, None, "f32", 1, False))

DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def bf(x):
    """round to bf16 (nearest even), keep the dtype"""
    return x.to(torch.bfloat16).to(x.dtype)


def _crc(*parts):
    return zlib.crc32(repr(parts).encode())


@functools.lru_cache(maxsize=2)
def operands(M, N, K, batch):
    """bf16-rounded A [batch, M, K] and B [batch, N, K] held as f32, sigma = K^-1/4 each (so that
    A.B has unit scale), with the float64 products A.B and S = |A|.|B| ([batch, M, N]).  Shared
    by every spec of one shape; do not modify."""
    g = torch.Generator().manual_seed(_crc("ab", M, N, K, batch))
    s = float(K) ** -0.25
    A = bf(s * torch.randn(batch, M, K, generator=g))
    B = bf(s * torch.randn(batch, N, K, generator=g))
    AB = torch.empty(batch, M, N, dtype=torch.float64)
    S = torch.empty(batch, M, N, dtype=torch.float64)
    step = max(1, (1 << 24) // max(K, 1))  # rows per block: 128 MiB of float64 A at a time
    for b in range(batch):
        Bd = B[b].double().t().contiguous()
        for r in range(0, M, step):
            Ad = A[b, r:r + step].double()
            AB[b, r:r + step] = Ad @ Bd
            S[b, r:r + step] = Ad.abs() @ Bd.abs()
    return A, B, AB, S


@functools.lru_cache(maxsize=2)
def make_case(spec):
    """The spec's tensors: A, B (operands()), bias f32 [N], aux bf16-rounded [batch, M, N] for
    the gradient activations, res1 / res2 [batch, M, N] (bf16-rounded where the spec says bf16)."""
    A, B, AB, S = operands(spec.M, spec.N, spec.K, spec.batch)
    g = torch.Generator().manual_seed(_crc("epi", tuple(spec)))
    shape = (spec.batch, spec.M, spec.N)
    bias = torch.randn(spec.N, generator=g) if spec.bias else None
    aux = bf(torch.randn(shape, generator=g)) if spec.act in GRAD_ACTS else None

    def res(kind):
        if kind is None:
            return None
        r = torch.randn(shape, generator=g)
        return bf(r) if kind == "bf16" else r
    return SimpleNamespace(spec=spec, A=A, B=B, AB=AB, S=S, bias=bias, aux=aux, res1=res(spec.res1),
                           res2=res(spec.res2))


# ----------------------------------------------------------------------------- activations
KB = math.sqrt(2.0 / math.pi)
KC = 0.044715


def gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(KB * (x + KC * x ** 3)))


def gelu_grad(x):
    t = torch.tanh(KB * (x + KC * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * KB * (1.0 + 3.0 * KC * x * x)


def qgelu(x):
    return x * torch.sigmoid(1.702 * x)


def qgelu_grad(x):
    s = torch.sigmoid(1.702 * x)
    return s + 1.702 * x * s * (1.0 - s)


def _sup(f, lo=-12.0, hi=12.0, n=480001):
    """largest |f| on a fine float64 grid, 1 % over for the grid step"""
    x = torch.linspace(lo, hi, n, dtype=torch.float64)
    return 1.01 * float(f(x).abs().max())


def _diff(f):
    h = 1e-5
    return lambda x: (f(x + h) - f(x - h)) / (2 * h)


# the largest slope of each function the epilogue evaluates on the computed value x
L_GELU = _sup(gelu_grad)            # 1.14
L_QGELU = _sup(qgelu_grad)          # 1.11
L_GELU_D = _sup(_diff(gelu_grad))   # |GELU''| <= 0.81: the slope of the aux_out of LTHM_ACT_GELU_D


def act_term(f, arg):
    """T of the bound: 8 x max |f in float32 - f in float64| over the case's arguments (float64
    tensor arg); the float32 run is the CPU's, the margin covers the device's exp and rcp."""
    if arg.numel() == 0:
        return 0.0
    return 8.0 * float((f(arg.float()).double() - f(arg)).abs().max())


# ----------------------------------------------------------------------------- reference
def reference(c, AB=None, dtype=torch.float64):
    """The epilogue in `dtype` (float64: the reference; float32: the CPU evaluation the host test
    accepts) on AB = A.B ([batch, M, N], default the case's float64 product).
    -> SimpleNamespace(x pre-activation, y after the activation, C before the cast, aux_out or None)"""
    s = c.spec
    AB = c.AB if AB is None else AB
    x = AB.to(dtype) * torch.tensor(s.alpha, dtype=dtype)
    if c.bias is not None:
        x = x + c.bias.to(dtype)
    aux_out = None
    if s.act == ACT_NONE:
        y = x
    elif s.act == ACT_GELU:
        y, aux_out = gelu(x), x
    elif s.act == ACT_QGELU:
        y, aux_out = qgelu(x), x
    elif s.act == ACT_GELU_D:
        y, aux_out = gelu(x), gelu_grad(x)
    elif s.act == ACT_GELU_GRAD:
        y = x * gelu_grad(c.aux.to(dtype))
    elif s.act == ACT_QGELU_GRAD:
        y = x * qgelu_grad(c.aux.to(dtype))
    elif s.act == ACT_MUL_AUX:
        y = x * c.aux.to(dtype)
    else:
        raise ValueError(s.act)
    C = y
    if c.res1 is not None:
        C = C + c.res1.to(dtype)
    if c.res2 is not None:
        C = C + c.res2.to(dtype)
    return SimpleNamespace(x=x, y=y, C=C, aux_out=aux_out)


def bound(c, ref=None):
    """Per-element error bounds (float64 [batch, M, N]) of C and of aux_out (None without one)
    against reference(c); the derivation is the module docstring's."""
    s = c.spec
    ref = reference(c) if ref is None else ref
    x = ref.x
    ex = abs(s.alpha) * (s.K + 1) * U32 * c.S
    if c.bias is not None:
        ex = ex + U32 * x.abs()
    ea = None
    if s.act == ACT_NONE:
        e = ex
    elif s.act in (ACT_GELU, ACT_GELU_D):
        e = L_GELU * ex + act_term(gelu, x)
        ea = ex if s.act == ACT_GELU else L_GELU_D * ex + act_term(gelu_grad, x)
    elif s.act == ACT_QGELU:
        e = L_QGELU * ex + act_term(qgelu, x)
        ea = ex
    elif s.act in (ACT_GELU_GRAD, ACT_QGELU_GRAD):
        f = gelu_grad if s.act == ACT_GELU_GRAD else qgelu_grad
        a = c.aux.double()
        e = f(a).abs() * ex + x.abs() * act_term(f, a) + U32 * ref.y.abs()
    else:  # ACT_MUL_AUX
        e = c.aux.double().abs() * ex + U32 * ref.y.abs()
    run = ref.y
    for r in (c.res1, c.res2):
        if r is not None:
            run = run + r.double()
            e = e + U32 * run.abs()
    if s.out_dtype == "bf16":
        e = e + U16 * (ref.C.abs() + e)
    if ea is not None:  # aux_out is bf16
        ea = ea + U16 * (ref.aux_out.abs() + ea)
    return e, ea


def ratio(got, ref, bnd):
    """max_ij |got - ref| / bound_ij (a NaN or an infinity in got gives inf)"""
    d = (got.double() - ref).abs()
    if not bool(torch.isfinite(d).all()):
        return float("inf")
    return float((d / bnd.clamp_min(1e-300)).max())


def evaluate_f32(c):
    """The case computed in float32 on the CPU (the matmul in float32, the epilogue in float32,
    the stores rounded as the spec says): what the bound must accept."""
    AB = torch.matmul(c.A, c.B.transpose(-1, -2))
    r = reference(c, AB=AB, dtype=torch.float32)
    C = bf(r.C) if c.spec.out_dtype == "bf16" else r.C
    return C, (bf(r.aux_out) if r.aux_out is not None else None)


# ----------------------------------------------------------------------------- memory layout
PATTERN = {torch.float32: 0x7FBADBAD, torch.bfloat16: 0x7FBA}  # NaN payloads no result takes
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
GUARD_ROWS = 1


def lds(s):
    """(lda, ldb, ldc, ldaux, ldr) of a spec"""
    return ((s.K if s.ka else s.M) + s.pad_a, (s.K if s.kb else s.N) + s.pad_b, s.N + s.pad_c, s.N + s.pad_aux,
            s.N + s.pad_r)


def strides(s):
    """(sA, sB, sC) batch strides in elements"""
    lda, ldb, ldc, _, _ = lds(s)
    return ((s.M if s.ka else s.K) * lda + s.pad_s, (s.N if s.kb else s.K) * ldb + s.pad_s,
            s.M * ldc + (s.pad_s + GUARD_ROWS * ldc if s.batch > 1 else 0))


def place(shape, ld, stride, off, dtype, values=None, kcontig=True):
    """A [batch, R, Cc] tensor laid out with row stride ld and batch stride `stride` behind a
    pointer offset of `off` elements (kcontig False: each batch entry stored transposed).
    -> (flat buffer of dtype holding `values` there and the guard pattern everywhere else, the
    element offset of the pointer, the index tensor [batch, R, Cc] of the elements in the buffer).
    At least one guard row lies in front of the first row and behind the last; with off = 0 the
    pointer is 32-byte aligned in a 32-byte aligned buffer."""
    batch, R, Cc = shape
    rows = R if kcontig else Cc
    base = off + (GUARD_ROWS * ld + 7) // 8 * 8
    n = base + (batch - 1) * stride + rows * ld + GUARD_ROWS * ld + 8
    b = torch.arange(batch)[:, None, None] * stride
    r = torch.arange(R)[None, :, None]
    cc = torch.arange(Cc)[None, None, :]
    idx = base + b + (r * ld + cc if kcontig else cc * ld + r)
    buf = torch.full((n,), PATTERN[dtype], dtype=INT_VIEW[dtype]).view(dtype)
    if values is not None:
        buf[idx.reshape(-1)] = values.reshape(-1).to(dtype)
    return buf, base, idx


def untouched(buf, idx):
    """every element of the flat buffer outside idx still holds the guard pattern, bit for bit"""
    iv = buf.view(INT_VIEW[buf.dtype]).clone()
    iv[idx.reshape(-1)] = PATTERN[buf.dtype]
    return torch.equal(iv, torch.full_like(iv, PATTERN[buf.dtype]))
