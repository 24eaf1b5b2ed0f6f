"""float64 reference of the optimizer step (clip_grad_norm_ -> Adam / AdamW / amsgrad -> EMA) and the per-element bounds an
fp32 implementation of it has to meet (tests/_optim_cases.py runs them on the HIP library and on the plain-C checker).

The reference is written from the semantics of torch.optim.Adam / AdamW (single-tensor step), of
torch.nn.utils.clip_grad_norm_ and of ExponentialMovingAverage.update, in numpy float64:

  clip      coef = max_norm / (sqrt(sum g^2) + 1e-6), clamped to at most 1 (a NaN stays a NaN);  g <- g * coef
  L2        g' = g + wd * p                      (Adam, weight_decay != 0)
  AdamW     p <- p * (1 - lr * wd)               (decoupled)
  moments   m <- lerp(m, g', 1 - b1);  v <- b2 * v + (1 - b2) * g'^2;  amsgrad: vmax <- max(vmax, v)
  update    p <- p - (lr / bc1) * m / (sqrt(v or vmax) / sqrt(bc2) + eps)
  ema       s <- s - (1 - decay) * (s - p)

Scalars.  Every scalar crosses the C ABI as a `float` (include/stk.h): lr, b1, b2, eps, weight_decay, bc1 = 1 - b1^t,
bc2 = 1 - b2^t, max_norm and one_minus_decay.  The reference therefore starts from np.float32(scalar), widened back to
float64, exactly the value the library receives; 1e-6 of the clip is the fp32 constant too.  This matters: 0.999 rounds
to 0.99900001287 in fp32, so 1 - b2 is 0.0009999871 for the library, -1.29e-5 relative to 0.001.  A float64 reference fed
the decimal betas sees a systematic -1.1e-5 relative bias in v after a few hundred steps, which is where the interface
rounds and not a kernel error (the weights b2 and 1 - b2 still sum to 1: 1 - b for b in [0.5, 1] is exact in fp32).

Bounds.  u = 2^-24 is the unit roundoff of fp32.  Division and sqrtf are IEEE-rounded in this build: csrc/Makefile
compiles with plain -O3 (no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt, whose default is the correctly
rounded form), and the checker is gcc -O2 -std=c11 without -ffast-math.  -ffp-contract may fuse a multiply into an add on
the device, which removes roundings and never adds one.  So every operation below counts as one rounding of relative size
u, and each bound is (number of roundings in the chain) x 2 x u x (the magnitude those roundings are relative to); the
factor 2 pays for second-order terms and for nothing else.  The counts:

  g     bit-equal when coef == 1.  Otherwise coef = fl(max_norm / fl(fl(sqrt(sumsq)) + 1e-6)) carries 3 roundings and
        g * coef one more (counted twice): |err| <= (2 + 3) u |g_ref|, with coef formed in float64 FROM THE SUMSQ THE
        LIBRARY PRODUCED, so that the error of the sum of squares (bounded on its own) is not charged again.
  g'    (L2 only) wd * p and the sum: 2 roundings relative to |g| + wd |p|:  d = 2 u (|g| + wd |p|)  (no factor 2: it is
        only used inside the bounds of m and v, which double it).
  m     m + (g' - m) * (1 - b1): the difference, 1 - b1, the product, the sum: 4 roundings, each relative to at most
        |m_old| + |g'|; L2 adds the 2 of g'.     |err| <= 2 (4 | 6) u (|m_old| + |g| + wd |p|)
  v     v * b2 + (1 - b2) * g' * g': per term at most 1 - b2, two products and the sum: 4 roundings relative to v_new (all
        terms are non-negative).                 |err| <= 8 u v_new   [+ 2 (1 - b2) (2 |g'| d + d^2) with L2: g' = g + wd p
                                                                        may cancel, and its absolute error d is squared]
  vmax  a selection between the old vmax (exact) and v: the bound of v, at vmax_new.
  dp    dp = p_new - p_old, formed in float64 from the library's output, against the reference dp = -A [- lr wd p_old],
        A = step_size * m_new / denom, denom = sqrt(v_new) / sqrt(bc2) + eps:
          step_size = fl(lr / bc1), the quotient m / denom and the product: 3 roundings          -> 6 u |A|
          denom: sqrtf, fl(sqrt(bc2)), the quotient, the sum with eps: 4 roundings               -> 8 u |A|
          the error of v under the root, halved by it                                             -> |A| bound(v) / (2 v_new)
          the error of m: it is relative to |m_old| + |g'|, NOT to |m_new| (m + (g' - m)(1 - b1) cancels when g' ~ -9 m), so
          it enters with its own magnitude                                                        -> step_size bound(m) / denom
          the final subtraction rounds at p's magnitude: half an ulp of p_new <= ulp(p_old)       -> ulp(p_old)
          AdamW: fl(lr * wd), fl(1 - .), fl(p * .): 3 roundings at p's magnitude                  -> 2 * 3 u |p_old|
        Without cancellation in m this is (6 + 8 + 4 + 8) u |dp_ref| + ulp(p_old), the c u |dp_ref| + ulp(p_old) form.
  ema   s - omd * (s - p): the difference, the product, the difference: |err| <= 3 u max(|s|, |p|)   (omd <= 1/2)
  sumsq relative error <= (k + 16) u, k = the longest per-thread accumulation chain (sumsq_chain below, from n and the
        grid rule of stk_sumsq_f32); the 16 covers what does not grow with n: the squares and the in-register tree of one
        float4 (3), the wave and workgroup reduction (6 + 3), the cast of the double second stage (1).
"""
import numpy as np

U = 2.0 ** -24
CLIP_EPS = np.float32(1e-6)


def f32(x):
  """The value a C `float` argument has: rounded to fp32, widened back to float64."""
  return float(np.float32(x))


class Hyper:
  """The scalars of one step as the ABI sees them (all rounded to fp32), t = the step number (1-based)."""

  def __init__(self, lr=2e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, adamw=False, t=1, max_norm=None, bc=None):
    self.args = dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd)
    self.adamw = bool(adamw)
    self.max_norm = max_norm                      # None: the library is called without sumsq
    # bias corrections as engine/optim.py forms them, in Python floats, then across the ABI as fp32
    self.bc1_arg, self.bc2_arg = bc if bc is not None else (1.0 - b1 ** t, 1.0 - b2 ** t)
    self.lr, self.b1, self.b2, self.eps, self.wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    self.bc1, self.bc2 = f32(self.bc1_arg), f32(self.bc2_arg)

  def abi_tail(self):
    """lr, b1, b2, eps, weight_decay, adamw, bc1, bc2 as passed to stk_adam_f32 (Python floats; ctypes rounds them)."""
    a = self.args
    return (a['lr'], a['b1'], a['b2'], a['eps'], a['wd'], int(self.adamw), self.bc1_arg, self.bc2_arg)


def clip_coef(sumsq, max_norm):
  """clip_grad_norm_'s coefficient in float64 from a sum of squares; NaN propagates (torch.clamp keeps it)."""
  with np.errstate(all='ignore'):
    coef = f32(max_norm) / (np.sqrt(np.float64(sumsq)) + np.float64(CLIP_EPS))
  if np.isnan(coef):
    return coef
  return min(coef, 1.0)


def adam_step(p, g, m, v, h, vmax=None):
  """One step in float64 on float64 arrays; g is the gradient AFTER clipping.  Returns a dict with the new state and the
  terms the bounds need."""
  p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
  ge = g + h.wd * p if (h.wd != 0.0 and not h.adamw) else g
  decay = -h.lr * h.wd * p if (h.wd != 0.0 and h.adamw) else np.zeros_like(p)
  m_new = m + (ge - m) * (1.0 - h.b1)
  v_new = h.b2 * v + (1.0 - h.b2) * ge * ge
  out = {'m': m_new, 'v': v_new, 'ge': ge}
  vd = v_new
  if vmax is not None:
    vd = np.maximum(np.asarray(vmax, np.float64), v_new)
    out['vmax'] = vd
  step_size = h.lr / h.bc1
  with np.errstate(all='ignore'):
    denom = np.sqrt(vd) / np.sqrt(h.bc2) + h.eps
    A = step_size * m_new / denom
  out.update(A=A, denom=denom, vd=vd, step_size=step_size, dp=decay - A, p=p + decay - A)
  return out


def ulp(x):
  return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def adam_bounds(p_old, g, m_old, h, ref):
  """name -> per-element bound of |library - reference| for one step (module text)."""
  p_old, g, m_old = (np.abs(np.asarray(a, np.float64)) for a in (p_old, g, m_old))
  l2 = h.wd != 0.0 and not h.adamw
  ge_abs = g + h.wd * p_old if l2 else g
  d = 2 * U * ge_abs if l2 else 0.0
  bm = 2 * (6 if l2 else 4) * U * (m_old + ge_abs)
  extra = 2 * (1.0 - h.b2) * (2 * np.abs(ref['ge']) * d + d * d) if l2 else 0.0
  bv = 8 * U * ref['v'] + extra
  b = {'m': bm, 'v': bv}
  bvd = bv
  if 'vmax' in ref:
    bvd = 8 * U * ref['vmax'] + extra
    b['vmax'] = bvd
  A = np.abs(ref['A'])
  with np.errstate(all='ignore'):
    root = np.where(ref['vd'] > 0, A * bvd / (2 * np.where(ref['vd'] > 0, ref['vd'], 1.0)), 0.0)
  b['dp'] = (6 + 8) * U * A + root + ref['step_size'] * bm / ref['denom'] + ulp(p_old)
  if h.wd != 0.0 and h.adamw:
    b['dp'] = b['dp'] + 6 * U * p_old
  return b


def clip_bound(g_ref):
  return 5 * U * np.abs(g_ref)


def ema_step(s, p, omd):
  s, p = np.asarray(s, np.float64), np.asarray(p, np.float64)
  return s - f32(omd) * (s - p)


def ema_bound(s, p):
  return 3 * U * np.maximum(np.abs(np.asarray(s, np.float64)), np.abs(np.asarray(p, np.float64)))


SUMSQ_BLOCKS, SUMSQ_PER_BLOCK = 1024, 256 * 16


def sumsq_grid(n):
  """Workgroups of 256 threads stk_sumsq_f32 launches: one per 4096 elements, at most 1024."""
  return min(max(-(-max(n, 1) // SUMSQ_PER_BLOCK), 1), SUMSQ_BLOCKS)


def sumsq_chain(n, vec):
  """The longest chain of `s +=` in one thread of the first stage: a grid-stride loop over float4s plus at most one tail
  element (16-byte aligned x), or over single floats."""
  threads = sumsq_grid(n) * 256
  if vec:
    return -(-(n // 4) // threads) + (1 if n % 4 else 0)
  return -(-n // threads)


def sumsq_ref(x):
  x = np.asarray(x, np.float64)
  return float(np.sum(x * x))


def sumsq_bound(n, vec):
  return (sumsq_chain(n, vec) + 16) * U
