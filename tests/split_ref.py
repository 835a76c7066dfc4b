"""CPU model of the split mode's operand planes and plane products (csrc/opload.h, csrc/common.h).

bf16 planes (split8 / split4): p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1), round to nearest
even each, every residual exact in fp32.  bf16 carries 8 significant bits (unit roundoff 2^-8), so
|x - p0| <= 2^-8 |x|, |x - p0 - p1| <= 2^-16 |x| and |x - p0 - p1 - p2| <= 2^-24 |x|.

Scaled fp16 pair (split8_h16, h16_pair): x' = x * 2^s (exact), h0 = fp16(x'), h1 = fp16(x' - h0).  fp16
carries 11 significant bits and its subnormals step by 2^-24, so |x' - h0 - h1| <= max(2^-22 |x'|, 2^-25).

Plane products: a kernel sums, per operand pair, the plane products
    NS = 2:  a0 b0 + a0 b1 + a1 b0                          (three MFMAs)
    NS = 3:  a0 b0 + a0 b1 + a1 b0 + a0 b2 + a2 b0 + a1 b1   (six MFMAs)
in fp32 accumulators.  plane_products() forms the same sums with every product and sum in float64: what the
kernel computes up to its fp32 accumulation, for any operation f(a, b) that is linear in each operand (a
matmul, the weight gradient of a convolution).
"""
import math

import torch

H16_WS = 10  # csrc/common.h: the exponent of weight planes made without an exponent table

PAIRS = {2: ((0, 0), (0, 1), (1, 0)), 3: ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))}


def planes_bf(x, n):
    """The n bf16 planes of a float32 tensor, each as float32 values."""
    assert x.dtype == torch.float32
    out, r = [], x
    for _ in range(n):
        p = r.to(torch.bfloat16).to(torch.float32)
        out.append(p)
        r = r - p  # exact in fp32
    return out


def h16_exp(mx):
    """opload.h h16_exp: s with mx * 2^s in [2^14, 2^15) for a finite mx > 0; 0 for mx == 0."""
    if not mx > 0.0:
        return 0
    return min(14 - (math.frexp(mx)[1] - 1), 126)


def planes_h16(x, s):
    """The scaled fp16 pair of a float32 tensor at exponent s, in the scaled units (float32 values)."""
    assert x.dtype == torch.float32
    v = x * (2.0 ** s)  # an exact power of two
    h0 = v.to(torch.float16).to(torch.float32)
    h1 = (v - h0).to(torch.float16).to(torch.float32)
    return [h0, h1]


def plane_products(f, a, b, ns):
    """sum over PAIRS[ns] of f(a_i, b_j) on the bf16 planes of float32 a and b, f evaluated in float64."""
    pa, pb = planes_bf(a, ns), planes_bf(b, ns)
    out = None
    for i, j in PAIRS[ns]:
        t = f(pa[i].double(), pb[j].double())
        out = t if out is None else out + t
    return out


def h16_products(f, a, b, sa=None, sb=H16_WS):
    """The three fp16 plane products of f(a, b) in float64, back in the units of a and b.  sa: the exponent
    of a's planes; None takes h16_exp(max |a|), the one exponent for the whole tensor -- the coarsest a
    running exponent ends at, so the kernels' per-block exponents are at least as fine."""
    if sa is None:
        sa = h16_exp(float(a.abs().max()))
    pa, pb = planes_h16(a, sa), planes_h16(b, sb)
    out = None
    for i, j in PAIRS[2]:
        t = f(pa[i].double(), pb[j].double())
        out = t if out is None else out + t
    return out * 2.0 ** -(sa + sb)


def rel_l2(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


def max_rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())
