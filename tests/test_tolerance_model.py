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

from _tolerances import PL_DGRAD_RTOL, PL_FWD_RTOL, PL_WGRAD_RTOL


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
