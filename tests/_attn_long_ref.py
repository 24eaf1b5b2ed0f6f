"""The streaming attention kernels (csrc/attention_long.hip, every T through the long entries and T > 256 through the MH
entries) per query row and per key column: the bounds and a numpy model of the streaming arithmetic.  The float64
reference, the metric and its helpers are those of tests/_attn_ref.py (reference, within, ratio, bound_of, floor_fraction,
pow2_scale_of, k_c); this module restates only what streaming changes.  Line numbers are those of attention_long.hip.

Metric.  |got - ref| <= (1 + 2^-4) (2^-24 Bu + F), element by element, as in _attn_ref.py: Bu a sum of absolute float64
terms times counts of roundings, F the floors of the fp16 split over exactly the extent each scale covers.  Every relative
error met below is under 2^-5 on every case (asserted: bounds()['rel']).  u = 2^-24, n_ch = ceil(T / 32) chunks (KC, l. 45).

Scores.  As the short kernels: s = us * acc (l. 280), us = scale / (sq sk) one rounding of scale times a power of two:
  E_s = (k_c(d) + 1) u S_abs + F_s,  F_s = scale (f_q sum_c |k| + f_k sum_c |q|),  f_x = 2^-25 / pow2_scale_of(max |x|) over
  the WHOLE tensor (amax_kernel's records, l. 58-76: one scale per tensor, all images and heads).

Online softmax (fwd_kernel, l. 266-303).  A key t' of chunk c enters o and l with the weight
  expf(x - m_c) * alpha_{c+1} * ... * alpha_{n_ch},  alpha_j = expf(m_{j-1} - m_j)          (l. 286, 290, 294, 300)
against exp(s - m) with the final maximum m.  The arguments' roundings are u |x - m_c| and u |m_{j-1} - m_j|; the maxima
only rise, so the differences telescope to u (m - x) = u |s - max s| <= u (S_abs + |max s|), the short kernels' term.  Each
of the at most n_ch functions is within K_FN u (the first chunk's alpha is expf(-inf) = 0 exactly).  So a term's relative
  r = E_s + u (S_abs + |max s|) + n_ch K_FN u = ((k_c(d) + 2) S_abs + |max s| + n_ch K_FN) u + F_s.
  l     8 adds per chunk in a lane (l. 291), the fma chain l = fma(l, alpha, ps) of n_ch roundings (l. 294), two shuffles
        (l. 304-305): K_L = 8 + n_ch + 2 in place of K_RED.
  o     `o *= alpha` rounds every earlier term once per chunk (l. 300): n_ch; the contraction is 3 * 32 fp16 products per
        chunk over n_ch chunks: k_c(32 n_ch); the reciprocal (l. 307; sv 2^13 l is l times a power of two) K_FN, `inv * o`
        (l. 312) 1:  k_o = k_c(32 n_ch) + n_ch + K_L + K_FN + 1 on sum p |v|, and r, rbar = sum p r as in _attn_ref.py.
        Floors: F_s through r and rbar, f_v, and the probabilities' split at 2^13 (l. 292, 297).  That split acts on
        exp(x - m_c) with m_c <= m, so the chunk's values are at least as large as exp(s - m) and as finely resolved: the
        short term 2^-38 sum |v| / sum exp(s - max s) is an upper bound (alpha <= 1 only shrinks an earlier chunk's residual).
  lse   = m + logf(l) (l. 313): rbar u (the scores), K_L u (the sum), K_FN u log T, u (|max s| + log T) (the addition).
Backward.  p = expf(us * acc - lse) (l. 360, 440) with the forward's lse: rb = E_s + E_lse + u S_abs + u |s - lse| + K_FN u
  as in _attn_ref.py with log T for log 256.  dp = ud * acc, ud = 1 / (sv sd) a power of two: E_dp = k_c(d) u DP_abs + F_dp.
  delta  is NOT sum p dp here: delta_kernel (l. 128-135) computes sum_c d_o o over the head's d channels by __fmaf_rn from
         the o the forward wrote:  E_delta = d u sum_c |d_o| |o| + sum_c |d_o| E_o  (E_o: the bound of o above, both parts).
         It enters E_ds for every key of the row.
  ds     = p * (ud * dp - delta) (l. 361, 441) carries no scale: the subtraction and the product are 2 roundings.  scale
         enters through the epilogue factor f = (scale / sk) / sig (l. 374; (scale / sq) / sig in DKV, l. 459): one rounding
         of scale times powers of two.  With the reference's ds = scale p (dp - delta):
           E_ds = scale p (|dp - delta| (rb + 3 u) + E_dp + E_delta[t]).
         ds is scaled per OWNED COLUMN (ds_rescale, l. 219-234): a query in DQ, a key in DKV, within one (image, head); the
         scale is the power of two of the running maximum, the accumulator is multiplied by the exact power-of-two ratio
         when it drops (l. 227-229).  A chunk is split at the scale of the maximum so far, which is at least as fine as the
         final one: the floor is f_ds = 2^-37 max (|ds| + E_ds) over the column (twice 2^-38, as in _attn_ref.py).  The
         maximum is that of the COMPUTED ds: where p (dp - delta) cancels (the peak of a one-hot row: the true ds is e^-100,
         the computed one E_dp + E_delta) the error of one entry sets the scale of its whole column, and |ds| alone would
         miss it.
  dq[c, t]  = f * acc (l. 381): (k_c(32 n_ch) + 1) u sum |k| |ds| + sum_t' |k| E_ds; floors f_k sum_t' |ds| + f_ds[t] sum_t' |k|.
  dk[c, t'] the same with q, the sum over t and f_ds[t'].
  dv[c, t'] = fv * acc, fv a power of two: sum_t |d_o| p (k_c(32 n_ch) u + rb); floors f_do sum_t p + 2^-38 sum_t |d_o|.
  beta != 0 as in _attn_ref.py: 2 u (|beta g0| + |v|).
Tiny values.  Every output carries 2^-149 (a result in the subnormal range is rounded to that step).  dq and dk carry more:
  the epilogue factor f = (scale / s_x) / sig is itself subnormal once s_x sig > scale 2^126, and is then a multiple of 2^-149:
  |f - f_true| <= 2^-150, a relative 2^-150 / f_true of the whole result, on sum |x| |ds|.  f_true is taken with the float64
  column maximum; the computed one may sit a binade lower, so the term is 2^-149 / f_true wherever f_true < 2^-125, else
  nothing.  And a chunk whose computed |ds| all lie under 2^-126 sets no scale (ds_rescale, l. 223): while its column has
  none its entries are split as they stand and vanish, an error of up to 2^-126 an entry: scale 2^-126 sum |x| over the
  stream.  (pow2_scale_of of a subnormal maximum is 1, and a scale only ever drops: in the parent such a chunk pinned its
  column's scale at 1 for good, and every later entry lost what lies under 2^-25.  Mutant 'a subnormal maximum sets the
  scale', caught by 'peaked'.)
  (The parent's factor scale / (s_x sig) was 0 there: s_x sig overflowed.  Mutant 'f of the overflowing product'.)

The model (model()) is numpy in float32 / float16: tensor scales from the whole tensor, hi / lo planes, three products
accumulated in float32, chunks of 32 keys (queries for DKV), the running maximum with the alpha rescale of o and of the
four lanes' l, the running per-column ds scale with its power-of-two rescale, delta by an fma chain from the model's own
o.  No waves, tiles, LDS or padding beyond the chunk.  Its `mutant` argument breaks it in the ways MUTANTS lists."""
import math

import numpy as np

import _attn_ref as ar
from _attn_ref import HALF_STEP, K_FN, P_SCALE, U, heads_view, k_c, pow2_scale_of

KC = 32
TINY = 2.0 ** -149
MUTANTS = ('mask admits T', 'last chunk dropped', 'alpha on o only', 'alpha on l only', 'no rescale when the ds scale drops',
           'ds scale of the first chunk', 'ds scale of the image', 'delta of the neighbouring head',
           'lse of the neighbouring head', 'head offset with C in CF', 'head offset with C in the output', 'hi lo dropped',
           'beta_k and beta_v exchanged', 'f of the overflowing product', 'a subnormal maximum sets the scale')


def n_chunks(T):
  return -(-T // KC)


def k_l(T):
  return 8.0 + n_chunks(T) + 2.0


def pow2_scale_arr(m):
  """_attn_ref.pow2_scale_of on an array of float32 maxima."""
  be = ((np.asarray(m, np.float32).view(np.uint32) >> 23) & 0xff).astype(np.int64)
  e = np.clip(127 + 13 - (be - 127), 1, 254) - 127
  return np.where(be == 0, 1.0, np.exp2(e.astype(np.float64))).astype(np.float32)


# ---- the bounds ------------------------------------------------------------------------------------------------------------
def bounds(ref, q, k, v, do, heads, scale, betas=(0.0, 0.0, 0.0), g0=None):
  """{output: (Bu, F)} as _attn_ref.bounds, for the streaming kernels (module text); 'rel' is the largest relative error the
  derivation meets."""
  B, C, T = q.shape
  d, n, log_t = C // heads, n_chunks(T), math.log(T)
  aq, ak, av, ado = (np.abs(heads_view(np.asarray(t, np.float64), heads)) for t in (q, k, v, do))
  s_of = {m: pow2_scale_of(np.abs(t).max()) for m, t in (('q', q), ('k', k), ('v', v), ('do', do))}
  f = {m: HALF_STEP / s for m, s in s_of.items()}
  a = ref['aux']
  p, S, DP, dp = a['p'], a['S_abs'], a['DP_abs'], a['dp']
  amax = np.abs(a['max_s'])
  cq, ck, cv, cdo = (t.sum(2) for t in (aq, ak, av, ado))                       # sums over channels: [B, H, T]

  Es_u, Es_f = (k_c(d) + 1) * S, scale * (f['q'] * ck[:, :, None, :] + f['k'] * cq[..., None])
  r_u, r_f = Es_u + S + amax[..., None] + K_FN * n, Es_f
  rbar_u, rbar_f = (p * r_u).sum(-1), (p * r_f).sum(-1)
  lse_u, lse_f = rbar_u + k_l(T) + K_FN * log_t + amax + log_t, rbar_f
  k_o = k_c(KC * n) + n + k_l(T) + K_FN + 1
  o_u = np.einsum('bhts,bhcs->bhct', p * (k_o + r_u + rbar_u[..., None]), av)
  o_f = (np.einsum('bhts,bhcs->bhct', p * (r_f + rbar_f[..., None]), av) + f['v']
         + 2.0 ** -38 * av.sum(-1)[..., None] / a['sumexp'][:, :, None, :])
  out = {'lse': (lse_u, lse_f), 'o': (o_u, o_f)}

  rb_u = Es_u + lse_u[..., None] + 2 * S + amax[..., None] + log_t + K_FN
  rb_f = Es_f + lse_f[..., None]
  Edp_u, Edp_f = k_c(d) * DP, f['do'] * cv[:, :, None, :] + f['v'] * cdo[..., None]
  ao = np.abs(heads_view(ref['o'], heads))
  de_u, de_f = d * (ado * ao).sum(2) + (ado * o_u).sum(2), (ado * o_f).sum(2)
  out['delta'] = (de_u, de_f)
  g = np.abs(dp - ref['delta'][..., None])
  Eds_u = scale * p * (g * (rb_u + 3) + Edp_u + de_u[..., None])
  Eds_f = scale * p * (g * rb_f + Edp_f + de_f[..., None])
  ads = np.abs(a['ds'])
  cds = ads + U * Eds_u + Eds_f                                                 # what a computed |ds| can reach
  k_g = k_c(KC * n) + 1

  def tiny(colmax, s_x, mag):                                                   # module text, "Tiny values"
    sig = pow2_scale_arr((colmax / scale).astype(np.float32)).astype(np.float64)
    f_true = scale / (s_x * sig)
    return np.where(f_true < 2.0 ** -125, 2.0 ** -149 / f_true, 0.0)[:, :, None, :] * mag

  kds, qds = np.einsum('bhcs,bhts->bhct', ak, ads), np.einsum('bhct,bhts->bhcs', aq, ads)
  out['dq'] = (k_g * kds + np.einsum('bhcs,bhts->bhct', ak, Eds_u),
               np.einsum('bhcs,bhts->bhct', ak, Eds_f) + f['k'] * ads.sum(3)[:, :, None, :]
               + 2.0 ** -37 * cds.max(3)[:, :, None, :] * ak.sum(-1)[..., None] + tiny(ads.max(3), s_of['k'], kds)
               + scale * 2.0 ** -126 * ak.sum(-1)[..., None])
  out['dk'] = (k_g * qds + np.einsum('bhct,bhts->bhcs', aq, Eds_u),
               np.einsum('bhct,bhts->bhcs', aq, Eds_f) + f['q'] * ads.sum(2)[:, :, None, :]
               + 2.0 ** -37 * cds.max(2)[:, :, None, :] * aq.sum(-1)[..., None] + tiny(ads.max(2), s_of['q'], qds)
               + scale * 2.0 ** -126 * aq.sum(-1)[..., None])
  out['dv'] = (np.einsum('bhct,bhts->bhcs', ado, p * (k_c(KC * n) + rb_u)),
               np.einsum('bhct,bhts->bhcs', ado, p * rb_f) + f['do'] * p.sum(2)[:, :, None, :]
               + 2.0 ** -38 * ado.sum(-1)[..., None])
  for m in ('o', 'dq', 'dk', 'dv'):
    out[m] = tuple(t.reshape(B, C, T) for t in out[m])
  for m in ar.OUTPUTS:
    out[m] = (out[m][0], out[m][1] + TINY)
  for i, m in enumerate(('dq', 'dk', 'dv')):
    if betas[i] != 0.0:
      out[m] = (out[m][0] + 2 * (np.abs(betas[i] * np.asarray(g0[i], np.float64)) + np.abs(ref[m])), out[m][1])
  out['rel'] = float(max((U * r_u + r_f).max(), (U * rb_u + rb_f).max()))
  return out


# ---- the numpy model -------------------------------------------------------------------------------------------------------
def _mma(acc, x, y, drop):
  """acc[g, i, j] += sum_n x[g, n, i] y[g, n, j] from (hi, lo) pairs: lo hi + hi lo + hi hi, float32, n after n, in place."""
  (xh, xl), (yh, yl) = x, y
  for n in range(xh.shape[1]):
    a_h, a_l, b_h, b_l = xh[:, n, :, None], xl[:, n, :, None], yh[:, n, None, :], yl[:, n, None, :]
    acc += a_l * b_h
    if not drop:
      acc += a_h * b_l
    acc += a_h * b_h


def _fma(a, b, c):
  """float32 fma(a, b, c) through float64 (the product is exact there)."""
  return (a.astype(np.float64) * b + c).astype(np.float32)


def _ds_stream(ds, x, chunks, mutant, drop):
  """The owned-column accumulation of DQ (columns: queries, stream: keys) and DKV (the reverse).  ds [G, columns, stream],
  x the (hi, lo) planes of the streamed operand as [G, stream, c] -> acc [G, c, columns] and the columns' scales sig."""
  f32 = np.float32
  G, ncol, _ = ds.shape
  acc, sig = np.zeros((G, x[0].shape[2], ncol), f32), np.zeros((G, ncol), f32)
  if mutant == 'ds scale of the image':
    sig = np.repeat(pow2_scale_arr(np.abs(ds).max((1, 2)))[:, None], ncol, 1)
  for j0 in chunks:
    blk = ds[:, :, j0:j0 + KC]
    dmax = np.abs(blk).max(-1)
    sc = pow2_scale_arr(dmax)
    some = dmax > 0 if mutant == 'a subnormal maximum sets the scale' else dmax >= f32(2.0 ** -126)
    if mutant == 'ds scale of the image':
      upd = np.zeros_like(dmax, bool)
    elif mutant == 'ds scale of the first chunk':
      upd = some & (sig == 0)
    else:
      upd = some & ((sig == 0) | (sc < sig))
    if mutant != 'no rescale when the ds scale drops':
      acc *= np.where(upd & (sig != 0), sc / np.where(sig == 0, f32(1), sig), f32(1)).astype(f32)[:, None, :]
    sig = np.where(upd, sc, sig)
    use = np.where(sig == 0, f32(1), sig)
    dh, dl = ar._split(blk, use[..., None])
    t_ = lambda z: np.ascontiguousarray(z.transpose(0, 2, 1))
    _mma(acc, tuple(z[:, j0:j0 + KC] for z in x), (t_(dh), t_(dl)), drop)
  return acc, sig


def model(q, k, v, do, heads, scale, betas=(0.0, 0.0, 0.0), g0=None, mutant=None):
  """The arithmetic of attention_long.hip on float32 [B, C, T] arrays (module text) -> the six outputs, float32.
  mutant: one of MUTANTS."""
  assert mutant is None or mutant in MUTANTS, mutant
  with np.errstate(over='ignore', invalid='ignore', divide='ignore', under='ignore'):
    return _model(q, k, v, do, heads, scale, betas, g0, mutant)


def _model(q, k, v, do, heads, scale, betas, g0, mutant):
  B, C, T = q.shape
  d, G, n = C // heads, B * heads, n_chunks(T)
  Tc = n * KC
  f32 = np.float32
  sc = {m: f32(pow2_scale_of(np.abs(t).max())) for m, t in (('q', q), ('k', k), ('v', v), ('do', do))}

  def hv(x, cf=False):                                     # [G, d, Tc], zeros past T
    x = heads_view(np.asarray(x, f32), heads)
    if cf and mutant == 'head offset with C in CF':        # head n of image b read a whole image per head on: (b + n, head 0)
      y = np.zeros_like(x)
      for b in range(B):
        for h in range(heads):
          if b + h < B:
            y[b, h] = x[b + h, 0]
      x = y
    return np.concatenate([x.reshape(G, d, T), np.zeros((G, d, Tc - T), f32)], 2)

  t_ = lambda z: np.ascontiguousarray(z.transpose(0, 2, 1))
  pl = {m: ar._split(hv(x), sc[m]) for m, x in (('q', q), ('k', k), ('v', v), ('do', do))}          # PF: [G, d, Tc]
  cf = {m: ar._split(hv(x, True), sc[m]) for m, x in (('q', q), ('k', k), ('v', v), ('do', do))}    # CF operands
  plT = {m: tuple(t_(z) for z in x) for m, x in pl.items()}                                         # [G, Tc, d]
  drop = mutant == 'hi lo dropped'
  chunks = [j0 for j0 in range(0, T, KC) if mutant != 'last chunk dropped' or j0 + KC <= T]
  us, ud = f32(scale) / (sc['q'] * sc['k']), f32(1) / (sc['v'] * sc['do'])
  s = us * ar._contract(tuple(z[:, :, :T] for z in cf['q']), cf['k'], drop)     # [G, t, t' < Tc]
  key_live = np.arange(Tc) < T
  # forward
  m_, l, acc = np.full((G, T), -np.inf, f32), np.zeros((G, T, 4), f32), np.zeros((G, d, T), f32)
  for j0 in chunks:
    live = key_live[j0:j0 + KC] | (mutant == 'mask admits T')
    x = np.where(live, s[:, :, j0:j0 + KC], f32(-np.inf))
    mn = np.maximum(m_, x.max(-1))
    alpha = np.exp(m_ - mn).astype(f32)
    p = np.exp(x - mn[..., None]).astype(f32)
    lanes = p.reshape(G, T, 2, 4, 4)                       # [u, g, e]: lane g adds its 8 values one after the other
    ps = np.zeros((G, T, 4), f32)
    for u_ in range(2):
      for e in range(4):
        ps = ps + lanes[:, :, u_, :, e]
    l = l + ps if mutant == 'alpha on o only' else _fma(l, alpha[..., None], ps)
    m_ = mn
    if mutant != 'alpha on l only':
      acc *= alpha[:, None, :]
    ph, plo = ar._split(p, P_SCALE)
    _mma(acc, tuple(z[:, j0:j0 + KC] for z in plT['v']), (t_(ph), t_(plo)), drop)
  lsum = (l[..., 0] + l[..., 1]) + (l[..., 2] + l[..., 3])
  o = (f32(1) / (sc['v'] * f32(P_SCALE) * lsum))[:, None, :] * acc
  lse = (m_ + np.log(lsum)).astype(f32)
  # backward
  nb = lambda z: np.roll(z.reshape(B, heads, T), 1, 1).reshape(G, T)
  do_f = hv(do)[:, :, :T]
  delta = np.zeros((G, T), f32)
  for c in range(d):
    delta = _fma(do_f[:, c], o[:, c], delta)
  de = nb(delta) if mutant == 'delta of the neighbouring head' else delta
  lse_b = nb(lse) if mutant == 'lse of the neighbouring head' else lse
  pb = np.where(key_live, np.exp(s - lse_b[..., None]), 0).astype(f32)
  dp = ud * ar._contract(tuple(z[:, :, :T] for z in cf['do']), cf['v'], drop)
  ds = (pb * (dp - de[..., None])).astype(f32)             # [G, t, t' < Tc]: no scale (it is in the epilogue factor)

  def factor(s_x, sig):
    if mutant == 'f of the overflowing product':
      f = f32(scale) / (s_x * sig)
    else:
      f = (f32(scale) / s_x) / sig
    return np.where(sig == 0, f32(0), f).astype(f32)

  aq_, sigq = _ds_stream(ds, plT['k'], chunks, mutant, drop)
  dq = factor(sc['k'], sigq)[:, None, :] * aq_
  pad_t = lambda z: np.concatenate([z, np.zeros(z.shape[:2] + (Tc - T,), f32)], 2)
  ak_, sigk = _ds_stream(pad_t(t_(ds[:, :, :T])), plT['q'], chunks, mutant, drop)
  dk = factor(sc['q'], sigk)[:, None, :] * ak_
  av_ = np.zeros((G, d, T), f32)
  pbT = pad_t(t_(pb[:, :, :T]))                            # [G, t', t < Tc]
  for j0 in chunks:
    ph, plo = ar._split(pbT[:, :, j0:j0 + KC], P_SCALE)
    _mma(av_, tuple(z[:, j0:j0 + KC] for z in plT['do']), (t_(ph), t_(plo)), drop)
  dv = (f32(1) / (sc['do'] * f32(P_SCALE))) * av_
  out = {'o': o, 'dq': dq, 'dk': dk, 'dv': dv}
  init = {'o': np.full((B, C, T), np.nan, f32), 'dq': g0[0], 'dk': g0[1], 'dv': g0[2]} if g0 is not None else None
  bq, bk, bv = betas
  if mutant == 'beta_k and beta_v exchanged':
    bk, bv = bv, bk
  for m, beta in (('o', 0.0), ('dq', bq), ('dk', bk), ('dv', bv)):
    t = out[m].astype(f32).reshape(B, C, T)
    if beta != 0.0:
      t = (np.float64(beta) * np.asarray(g0[('dq', 'dk', 'dv').index(m)], np.float64) + t.astype(np.float64)).astype(f32)
    if mutant == 'head offset with C in the output':       # pair (b, h) written where (b + h, head 0) lies
      w = heads_view(np.array(init[m], f32), heads)
      src = heads_view(t, heads)
      for b in range(B):
        for h in range(heads):
          if b + h < B:
            w[b + h, 0] = src[b, h]
      t = w.reshape(B, C, T)
    out[m] = t
  out['lse'], out['delta'] = lse.reshape(B, heads, T), delta.reshape(B, heads, T)
  return out
