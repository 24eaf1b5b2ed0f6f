"""The contraction bounds of tests/_tolerances.py against a numpy model of the planes split (CPU).

The plane-operand kernels scale each operand by a power of two (max |.| into [2^13, 2^14)), split every value into two
fp16 terms hi + lo, and form each fp32 product from three of the four cross terms (hi hi + hi lo + lo hi; lo lo is below
fp32 rounding).  The model does the same on GEMMs with the accumulation lengths of the tested shapes and checks that the
bounds sit between a correct split and a broken one: the correct product lands at <= 1/10 of the bound, and each mutation
a kernel could plausibly carry (a cross term lost, the lo plane at the wrong weight, a K-split slab not summed) lands at
>= 5x the bound.  A later edit that loosens a bound past what catches these fails here, without a GPU.

The products are exact (fp16 x fp16 fits an fp32 mantissa) and are summed in float64 here, so the model isolates what
the split itself loses; fp32 accumulation on the device adds to it, which is what the GPU measurement bounds."""
import numpy as np
import pytest

from _tolerances import (F32_DGRAD_RTOL, F32_FWD_RTOL, F32_GEMM_RTOL, F32_WGRAD_RTOL, PL_DGRAD_RTOL, PL_FWD_RTOL,
                         PL_WGRAD_RTOL)


def _split(a):
  """hi, lo planes of s a (float64 arrays holding fp16 values) and the scale s, as stk_split_planes_f32."""
  a = a.astype(np.float32)
  m = float(np.abs(a).max())
  s = 1.0 if m == 0 else 2.0 ** (13 - int(np.floor(np.log2(m))))
  xs = a * np.float32(s)
  hi = xs.astype(np.float16)
  lo = (xs - hi.astype(np.float32)).astype(np.float16)
  return hi.astype(np.float64), lo.astype(np.float64), s


def _model(w, x, slabs):
  """C = w @ x through the planes of both operands, K split into `slabs` partial sums.  Returns the float64 reference and
  one result per variant (max|err| / max|ref| each)."""
  wh, wl, sw = _split(w)
  xh, xl, sx = _split(x)
  K = w.shape[1]
  edges = np.linspace(0, K, slabs + 1).astype(int)

  def prod(a, b):           # [slab, M, N] partial products
    return np.stack([a[:, lo:hi] @ b[lo:hi] for lo, hi in zip(edges[:-1], edges[1:])])

  hh, hl, lh = prod(wh, xh), prod(wh, xl), prod(wl, xh)
  ref = w.astype(np.float64) @ x.astype(np.float64)
  unscale = 1.0 / (sw * sx)
  variants = {
    'correct': hh + hl + lh,
    'cross term dropped': hh + hl,
    'lo plane at half weight': hh + 0.5 * hl + lh,
    'lo scale off by 2x': hh + 2.0 * hl + lh,
    'slab dropped': (hh + hl + lh)[:-1],
  }
  scale = np.abs(ref).max()
  return {k: float(np.abs(v.sum(0) * unscale - ref).max() / scale) for k, v in variants.items()}


# (bound, accumulation length K, K-split slabs of the device plan, per-column magnitude spread in decades)
MODEL_CASES = [
  ('fwd', PL_FWD_RTOL, 128 * 9, 3, 0),         # 128 -> 128 3x3 (K split 3 at batch 8, 32 x 32)
  ('fwd', PL_FWD_RTOL, 256 * 9, 6, 0),         # 256 -> 256 3x3 (K split 6 at batch 4, 32 x 32 and batch 128, 4 x 4)
  ('fwd', PL_FWD_RTOL, 256, 1, 0),             # 1x1 / NIN
  ('dgrad', PL_DGRAD_RTOL, 256 * 9, 4, 4),     # 256 -> 256 at 8 x 8, dy spread over 4 decades per image
  ('dgrad', PL_DGRAD_RTOL, 128 * 9, 1, 0),
  ('wgrad', PL_WGRAD_RTOL, 128 * 1024, 32, 4), # 128 -> 128 at 32 x 32, batch 128: K = N H W
  ('wgrad', PL_WGRAD_RTOL, 128 * 64, 8, 4),    # 256 -> 256 at 8 x 8, batch 128
  ('wgrad', PL_WGRAD_RTOL, 128 * 16, 4, 0),    # 4 x 4
]


@pytest.mark.parametrize('case', MODEL_CASES, ids=lambda c: f'{c[0]}_K{c[2]}_s{c[3]}_d{c[4]}')
def test_bound_separates_correct_split_from_mutations(case):
  what, bound, K, slabs, decades = case
  rng = np.random.default_rng(K + slabs)
  M, Nc = 48, 40
  w = rng.standard_normal((M, K)).astype(np.float32) / np.float32(np.sqrt(K))
  x = rng.standard_normal((K, Nc)).astype(np.float32)
  if decades:
    if what == 'wgrad':       # the K axis runs over images: dy rows scaled per image, as the loss weights make them
      x *= np.logspace(-decades, 0, 16).repeat(K // 16).astype(np.float32)[:, None]
    else:                     # the N axis runs over images
      x *= np.logspace(-decades, 0, Nc).astype(np.float32)[None, :]
  err = _model(w, x, slabs)
  print(what, K, {k: f'{v:.2e}' for k, v in err.items()})
  assert err['correct'] <= bound / 10, (err['correct'], bound)
  for k, v in err.items():
    if k != 'correct' and not (k == 'slab dropped' and slabs == 1):
      assert v >= 5 * bound, (k, v, bound)


def test_model_split_is_the_library_format():
  """The model's split is the format's: hi + lo carries s x to 2^-22 relative, and the scale puts the maximum in
  [2^13, 2^14) -- including a maximum that is exactly a power of two (the floor(log2) edge)."""
  rng = np.random.default_rng(0)
  x = rng.standard_normal(4096).astype(np.float32)
  x[7] = 4.0
  x = np.clip(x, -4.0, 4.0)
  hi, lo, s = _split(x)
  assert s == 2.0 ** 11 and np.abs(hi).max() == 2.0 ** 13
  xs = x.astype(np.float64) * s
  assert np.all(np.abs(hi + lo - xs) <= np.maximum(np.abs(xs) * 2.0 ** -22, 2.0 ** -25))


# ---- the f32-operand contractions (F32_* bounds) ----------------------------------------------------------------------
# The f32-input MFMA kernels, wgrad9_kernel and stk_gemm_f32 multiply plain fp32 values and accumulate in fp32, one k chunk
# (36 wide for the 3x3 layers: 4 channels x 9 taps; 32 wide otherwise) after the other; a K split leaves one partial slab
# per split, and splitk_reduce_kernel sums the slabs in fp32 in ascending order.  The model: fp32 products, summed in fp32
# in k order inside a chunk, the chunk sums added in fp32 to the slab's accumulator, the slabs added in fp32.  It models
# how much rounding such an order collects, not the matrix core's exact order inside an instruction.
def _round_bits(a, bits):
  """a rounded to `bits` significant bits (round to nearest), exponent range untouched"""
  m, e = np.frexp(a.astype(np.float64))
  return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e).astype(np.float32)


def _f32_slabs(w, x, kc, slabs):
  """[slab, M, N] fp32 partial sums of w @ x; a slab is a whole number of k chunks, as the device plans split K"""
  K = w.shape[1]
  chunks = -(-K // kc)
  per = -(-chunks // slabs) * kc
  out = []
  for s0 in range(0, K, per):
    acc = np.zeros((w.shape[0], x.shape[1]), np.float32)
    for k0 in range(s0, min(s0 + per, K), kc):
      part = np.zeros_like(acc)
      for k in range(k0, min(k0 + kc, s0 + per, K)):
        part += w[:, k, None] * x[None, k, :]
      acc += part
    out.append(acc)
  assert len(out) == slabs, (len(out), slabs)
  return np.stack(out)


def _f32_sum(slabs):
  acc = np.zeros_like(slabs[0])
  for s in slabs:
    acc += s
  return acc


def _f32_model(w, x, kc, slabs):
  ref = w.astype(np.float64) @ x.astype(np.float64)
  part = _f32_slabs(w, x, kc, slabs)
  variants = {'correct': _f32_sum(part),
              'operands at 11 bits': _f32_sum(_f32_slabs(_round_bits(w, 11), _round_bits(x, 11), kc, slabs))}
  if w.shape[1] % kc:
    variants['last k of the ragged chunk dropped'] = _f32_sum(_f32_slabs(w[:, :-1], x[:-1], kc, slabs))
  if slabs > 1:
    variants['slab dropped'] = _f32_sum(part[:-1])
    variants['slab counted twice'] = _f32_sum(np.concatenate([part, part[-1:]]))
  scale = np.abs(ref).max()
  return {k: float(np.abs(v.astype(np.float64) - ref).max() / scale) for k, v in variants.items()}


# (bound, accumulation length K, k chunk, K-split slabs): the lengths of the cases of tests/test_gpu_f32_contractions.py
F32_MODEL_CASES = [
  ('fwd', F32_FWD_RTOL, 27, 36, 1),          # 3 -> 48 at stride 2
  ('fwd', F32_FWD_RTOL, 207, 36, 1),         # 23 -> 128
  ('fwd', F32_FWD_RTOL, 4608, 36, 1),        # 512 -> 32
  ('dgrad', F32_DGRAD_RTOL, 27, 36, 1),
  ('dgrad', F32_DGRAD_RTOL, 207, 36, 1),
  ('dgrad', F32_DGRAD_RTOL, 4608, 36, 1),
  ('gemm', F32_GEMM_RTOL, 33, 32, 1),
  ('gemm', F32_GEMM_RTOL, 512, 32, 1),
  ('wgrad', F32_WGRAD_RTOL, 8 * 1024, 32, 16),   # wgrad9_kernel<32>: K = N OH OW = 8192 in 16 slabs
  ('wgrad', F32_WGRAD_RTOL, 19 * 256, 32, 9),    # wgrad9_kernel<16>: 4864 in 9 slabs, the last short
  ('wgrad', F32_WGRAD_RTOL, 32 * 64, 32, 4),     # wgrad9_kernel<8>
  ('wgrad', F32_WGRAD_RTOL, 15 * 144, 32, 4),    # 128-wide generic kernel: 2160, not a multiple of the chunk
]


@pytest.mark.parametrize('case', F32_MODEL_CASES, ids=lambda c: f'{c[0]}_K{c[2]}_kc{c[3]}_s{c[4]}')
def test_f32_bound_separates_correct_accumulation_from_mutations(case):
  """Each F32_* bound sits between fp32 accumulation done right (<= 1/3 of it) and what a kernel could plausibly get
  wrong (>= 5x): the last element of a ragged K lost, a K-split slab not summed or summed twice, operands that went
  through a half-precision mantissa.  Loosening a bound to the old 1e-4 fails here, without a GPU."""
  what, bound, K, kc, slabs = case
  rng = np.random.default_rng(K + slabs)
  M, Nc = 48, 40
  w = rng.standard_normal((M, K)).astype(np.float32) / np.float32(np.sqrt(K))
  x = rng.standard_normal((K, Nc)).astype(np.float32)
  err = _f32_model(w, x, kc, slabs)
  print(what, K, {k: f'{v:.2e}' for k, v in err.items()})
  assert err['correct'] <= bound / 3, (err['correct'], bound)
  for k, v in err.items():
    if k != 'correct':
      assert v >= 5 * bound, (k, v, bound)
