"""The short-map attention kernels (csrc/attention.hip, T <= 256) per query row and per key column: a float64 reference
with the quantities the error bounds need, the bounds themselves, and a numpy model of the arithmetic (not of the kernel's
code) that has to stay inside half of every bound before anything runs on a GPU (tests/test_attention_cases_cpu.py).
tests/_mh_ref.py stays what the other tests import; reference() restates it head by head in numpy and is checked against it.

Metric.  |got - ref| <= (1 + 2^-4) (2^-24 Bu + F), element by element.  Bu is a sum of terms k_i B_i: each B_i is a sum of
absolute terms of the float64 reference and each k_i a count of roundings read from attention.hip; F is the floor, the
absolute error of the fp16 split where a value is too small next to the maximum of the extent that shares its scale.  The
factor 1 + 2^-4 is the second order: every relative error below is under 2^-5 on every case (asserted), so a product of two
of them is under 2^-5 of one.  within() reports err / bound and asserts <= 1; floor_fraction() is F / (2^-24 Bu + F).

Counts used throughout (u = 2^-24):
  split       split.h: v = s x (exact, s a power of two), hi = fp16(v), lo = fp16(v - hi): |v - hi - lo| <= 2^-22 |v| = 4 u |v|
              while lo is a normal fp16 number, else <= 2^-25 (half the fp16 subnormal step): the floor 2^-25 / s.
  product     hi hi + hi lo + lo hi (SA / SB of attn_kernel): 4 u for each operand's split and 4 u for the missing lo lo.
  k_c(n)      a contraction of n fp32 products = 3 n fp16 products accumulated in fp32 by the MFMAs, in some order:
              at most 3 n roundings on each term, so k_c(n) = 3 n + 12 on sum |x| |y|.
  K_FN = 2    expf, logf and 1.f / x are within one ulp = 2 u.
  K_RED = 24  col_reduce and the loops in front of it: 16 values a thread, the __shfl_xor partner, at most 7 more waves.

s[t, t'] (phase A and `us * acc`; us = scale / (sx sy) is one rounding of scale times a power of two, applied once):
  E_s = (k_c(d) + 1) u S_abs + F_s,   S_abs = scale sum_c |q| |k|,   F_s = scale (f_q sum_c |k[c, t']| + f_k sum_c |q[c, t]|),
  f_x = 2^-25 / pow2_scale_of(max |x|), the maximum over the WHOLE tensor, all images and heads (attn_amax_kernel's records).

Forward.  p' = expf(s - mx), mx the maximum of the computed scores.  Against exp(s - mx) with the true s, p' is off by the
relative r = E_s + u |s - mx| + K_FN u, and |s - mx| <= S_abs + |max s|:  r = ((k_c(d) + 2) S_abs + |max s| + K_FN) u + F_s.
  lse[t] = mx + logf(sum p'):  sum_t' p r (the scores), K_RED u (the sum), K_FN u log T (logf), u (|max s| + log T) (the
           addition).  The issue's structure sum p S_abs + |max s| + 1 with k = k_c(d) + 2 on the first, 2 on the second
           and K_RED + 3 log 256 on the third term.
  o[c, t]  = (1 / sum) / (sa 2^13) * sum_t' v p':  each term p |v| carries r[t, t'] (its p'), rbar[t] = sum_t'' p r (the
           row sum), and k_o = k_c(T) + K_RED + K_FN + 1 (contraction, row sum, reciprocal, the epilogue's `f * oacc`).
           Floors: F_s through r and rbar; f_v (the probabilities sum to 1); and the probabilities' own split at the fixed
           scale 2^13, which acts on p' = exp(s - mx) BEFORE the division: 2^-38 sum_t' |v[c, t']| / sum_t' exp(s - max s).
Backward.  p = expf(us * acc - lse) with the lse the forward wrote: rb = E_s + E_lse + u S_abs (us * acc) + u |s - lse|
           + K_FN u, |s - lse| <= S_abs + |max s| + log T.  dp = ud * acc (ud a power of two): E_dp = k_c(d) u DP_abs + F_dp,
           DP_abs = sum_c |do| |v|, F_dp = f_do sum_c |v[c, t']| + f_v sum_c |do[c, t]|.
  delta[t] = sum_t' p dp by __fmaf_rn and col_reduce:  sum_t' p (|dp| (K_RED u + rb) + E_dp).
  ds       = a.scale * (p * (dp - delta)): three roundings, so
           E_ds = scale p (|dp - delta| (rb + 3 u) + E_dp + E_delta[t]).   (The issue's |dp| + |delta| terms stand for the
           rounding of the subtraction; it is u |dp - delta|, which is smaller, and is in the 3 u.)
           ds is split at the scale of ITS workgroup's maximum (dmax, sred): 64 consecutive queries x all keys in DQ, 64
           consecutive keys x all queries in DKV.  Floor f_ds = 2^-37 max |ds| over that tile (twice 2^-38: pow2_scale_of
           of the computed maximum may sit one binade from that of the float64 one).
  dq[c, t]  = sum_t' k ds:  k_c(T) u sum |k| |ds| + sum_t' |k| E_ds;  floors f_k sum_t' |ds| + f_ds[tile of t] sum_t' |k[c, t']|.
              The epilogue multiplies by 1 / (sa sds), a power of two: exact.
  dk[c, t'] = sum_t q ds:   the same with q, the sum over t and the tile of t'.
  dv[c, t'] = sum_t do p:   sum_t |do| p (k_c(T) u + rb);  floors f_do sum_t p + 2^-38 sum_t |do[c, t]| (p at 2^13).
  beta != 0: out = fma(beta, g0, v), one rounding of the sum: u (|beta g0| + |v|), taken twice: a single rounding can
             reach its full u, and the model has to stay inside HALF of the bound.

The model (model()) is numpy in float32 / float16 with the same precisions: pow2_scale_of of the stated extent, hi / lo,
the three products accumulated in float32 one contracted index after the other, float32 exp / log, the row sum and delta
by float32 accumulation without fma at the depth K_RED counts (a plain chain of 256 would collect ten times the roundings
the kernel's reduction can), ds and its split at the tile scale.  No waves, tiles or LDS.  Its `mutant` argument breaks it
in the ways tests/test_attention_cases_cpu.py lists; every mutant has to land 5 bounds out on some case."""
import math

import numpy as np

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -4
K_FN, K_RED = 2.0, 24.0
LOG_T = math.log(256.0)
P_SCALE = 8192.0
HALF_STEP = 2.0 ** -25           # half the fp16 subnormal step
OUTPUTS = ('o', 'lse', 'delta', 'dq', 'dk', 'dv')


def k_c(n):
  return 3.0 * n + 12.0


def pow2_scale_of(m):
  """split2::pow2_scale_of (csrc/split.h) on a float32 maximum."""
  be = (int(np.float32(m).view(np.uint32)) >> 23) & 0xff
  if be == 0:
    return 1.0
  return float(2.0 ** (min(max(127 + 13 - (be - 127), 1), 254) - 127))


def heads_view(x, heads):
  B, C, T = x.shape
  return x.reshape(B, heads, C // heads, T)


# ---- the float64 reference -----------------------------------------------------------------------------------------------
def reference(q, k, v, do, heads, scale):
  """float64 attention of [B, C, T] arrays, all heads at once: the outputs (o, dq, dk, dv as [B, C, T]; lse, delta as
  [B, heads, T]) and, under 'aux', p, dp, ds, S_abs, DP_abs as [B, heads, T, T'] and max_s."""
  B, C, T = q.shape
  q, k, v, do = (heads_view(np.asarray(t, np.float64), heads) for t in (q, k, v, do))
  s = scale * np.einsum('bhct,bhcs->bhts', q, k)
  mx = s.max(-1)
  lse = mx + np.log(np.exp(s - mx[..., None]).sum(-1))
  p = np.exp(s - lse[..., None])
  dp = np.einsum('bhct,bhcs->bhts', do, v)
  delta = (p * dp).sum(-1)
  ds = scale * p * (dp - delta[..., None])
  out = {'o': np.einsum('bhts,bhcs->bhct', p, v), 'dq': np.einsum('bhcs,bhts->bhct', k, ds),
         'dk': np.einsum('bhct,bhts->bhcs', q, ds), 'dv': np.einsum('bhct,bhts->bhcs', do, p)}
  out = {n: t.reshape(B, C, T) for n, t in out.items()}
  out.update(lse=lse, delta=delta)
  out['aux'] = {'p': p, 'dp': dp, 'ds': ds, 'max_s': mx, 'sumexp': np.exp(lse - mx),
                'S_abs': scale * np.einsum('bhct,bhcs->bhts', np.abs(q), np.abs(k)),
                'DP_abs': np.einsum('bhct,bhcs->bhts', np.abs(do), np.abs(v))}
  return out


def tile_max(a, axis):
  """max of a [B, H, T, T'] array over 64-wide tiles of `axis` (2: queries, 3: keys) and the whole other axis, per element
  of `axis`: [B, H, T]."""
  m = a.max(5 - axis)
  T = m.shape[-1]
  out = np.empty_like(m)
  for n0 in range(0, T, 64):
    out[..., n0:n0 + 64] = m[..., n0:n0 + 64].max(-1, keepdims=True)
  return out


def bounds(ref, q, k, v, do, heads, scale, betas=(0.0, 0.0, 0.0), g0=None):
  """{output: (Bu, F)}: the rounding part in units of u and the floor, float64 arrays of the outputs' shapes (module text).
  'rel' is the largest relative error the derivation meets (the second-order check)."""
  B, C, T = q.shape
  d = C // heads
  aq, ak, av, ado = (np.abs(heads_view(np.asarray(t, np.float64), heads)) for t in (q, k, v, do))
  f = {n: HALF_STEP / pow2_scale_of(np.abs(t).max()) for n, t in (('q', q), ('k', k), ('v', v), ('do', do))}
  a = ref['aux']
  p, S, DP, dp = a['p'], a['S_abs'], a['DP_abs'], a['dp']
  amax = np.abs(a['max_s'])
  cq, ck, cv, cdo = (t.sum(2) for t in (aq, ak, av, ado))                       # sums over channels: [B, H, T]

  Es_u, Es_f = (k_c(d) + 1) * S, scale * (f['q'] * ck[:, :, None, :] + f['k'] * cq[..., None])
  r_u, r_f = Es_u + S + amax[..., None] + K_FN, Es_f
  rbar_u, rbar_f = (p * r_u).sum(-1), (p * r_f).sum(-1)
  lse_u, lse_f = rbar_u + K_RED + K_FN * LOG_T + amax + LOG_T, rbar_f
  k_o = k_c(T) + K_RED + K_FN + 1
  out = {'lse': (lse_u, lse_f)}
  out['o'] = (np.einsum('bhts,bhcs->bhct', p * (k_o + r_u + rbar_u[..., None]), av),
              np.einsum('bhts,bhcs->bhct', p * (r_f + rbar_f[..., None]), av) + f['v']
              + 2.0 ** -38 * av.sum(-1)[..., None] / a['sumexp'][:, :, None, :])

  rb_u = Es_u + lse_u[..., None] + 2 * S + amax[..., None] + LOG_T + K_FN
  rb_f = Es_f + lse_f[..., None]
  Edp_u, Edp_f = k_c(d) * DP, f['do'] * cv[:, :, None, :] + f['v'] * cdo[..., None]
  de_u = (p * (np.abs(dp) * (K_RED + rb_u) + Edp_u)).sum(-1)
  de_f = (p * (np.abs(dp) * rb_f + Edp_f)).sum(-1)
  out['delta'] = (de_u, de_f)
  g = np.abs(dp - ref['delta'][..., None])
  Eds_u = scale * p * (g * (rb_u + 3) + Edp_u + de_u[..., None])
  Eds_f = scale * p * (g * rb_f + Edp_f + de_f[..., None])
  ads = np.abs(a['ds'])
  f_dsq, f_dsk = 2.0 ** -37 * tile_max(ads, 2), 2.0 ** -37 * tile_max(ads, 3)
  out['dq'] = (np.einsum('bhcs,bhts->bhct', ak, k_c(T) * ads + Eds_u),
               np.einsum('bhcs,bhts->bhct', ak, Eds_f) + f['k'] * ads.sum(3)[:, :, None, :]
               + f_dsq[:, :, None, :] * ak.sum(-1)[..., None])
  out['dk'] = (np.einsum('bhct,bhts->bhcs', aq, k_c(T) * ads + Eds_u),
               np.einsum('bhct,bhts->bhcs', aq, Eds_f) + f['q'] * ads.sum(2)[:, :, None, :]
               + f_dsk[:, :, None, :] * aq.sum(-1)[..., None])
  out['dv'] = (np.einsum('bhct,bhts->bhcs', ado, p * (k_c(T) + rb_u)),
               np.einsum('bhct,bhts->bhcs', ado, p * rb_f) + f['do'] * p.sum(2)[:, :, None, :]
               + 2.0 ** -38 * ado.sum(-1)[..., None])
  for n in ('o', 'dq', 'dk', 'dv'):
    out[n] = tuple(t.reshape(B, C, T) for t in out[n])
  for i, n in enumerate(('dq', 'dk', 'dv')):
    if betas[i] != 0.0:
      out[n] = (out[n][0] + 2 * (np.abs(betas[i] * np.asarray(g0[i], np.float64)) + np.abs(ref[n])), out[n][1])
  out['rel'] = float(max((U * r_u + r_f).max(), (U * rb_u + rb_f).max()))
  return out


def bound_of(bnd, name):
  bu, fl = bnd[name]
  return SECOND_ORDER * (U * bu + fl)


def floor_fraction(bnd, name):
  bu, fl = bnd[name]
  return fl / np.maximum(U * bu + fl, 1e-300)


def ratio(got, want, bound):
  """err / bound element by element, inf where the result is not finite."""
  g = np.asarray(got, np.float64)
  r = np.abs(g - want) / np.maximum(bound, 1e-300)
  return np.where(np.isfinite(g), r, np.inf)


def within(got, want, bound, what, show=True):
  """tests/_stream_util.within on a bound that carries its floor: asserts err <= bound element by element, returns (and
  prints) the worst err / bound."""
  r = ratio(got, want, bound)
  worst = int(r.argmax())
  w = float(r.reshape(-1)[worst])
  if show:
    print(f'  {what}: worst err / bound {w:.3g}')
  idx = np.unravel_index(worst, r.shape)
  assert w <= 1.0, f'{what}: err / bound {w:.3g} ({int((r > 1).sum())} elements over) at {tuple(int(i) for i in idx)}: ' \
                   f'got {float(np.asarray(got).reshape(-1)[worst])!r}, want {float(np.asarray(want).reshape(-1)[worst])!r}'
  return w


# ---- the numpy model -----------------------------------------------------------------------------------------------------
def _split(x, s):
  """hi, lo of s x (float32 arrays holding fp16 values); s a float or an array of powers of two."""
  v = (x * np.asarray(s, np.float32)).astype(np.float32)
  hi = v.astype(np.float16)
  lo = (v - hi.astype(np.float32)).astype(np.float16)
  return hi.astype(np.float32), lo.astype(np.float32)


def _contract(x, y, drop_hl=False):
  """acc[g, i, j] = sum_n x[g, n, i] y[g, n, j] from (hi, lo) pairs: lo hi + hi lo + hi hi, float32, n after n."""
  (xh, xl), (yh, yl) = x, y
  acc = np.zeros((xh.shape[0], xh.shape[2], yh.shape[2]), np.float32)
  for n in range(xh.shape[1]):
    a_h, a_l, b_h, b_l = xh[:, n, :, None], xl[:, n, :, None], yh[:, n, None, :], yl[:, n, None, :]
    acc += a_l * b_h
    if not drop_hl:
      acc += a_h * b_l
    acc += a_h * b_h
  return acc


def _reduce(a):
  """float32 sum over the last axis with the depth of the kernel's reduction (K_RED): runs of 16 one element after the
  other, two runs added, the pairs one after the other."""
  n = a.shape[-1]
  a = np.concatenate([a, np.zeros(a.shape[:-1] + (-n % 32,), np.float32)], -1).reshape(a.shape[:-1] + (-1, 2, 16))
  run = np.zeros(a.shape[:-1], np.float32)
  for j in range(16):
    run = run + a[..., j]
  pair = run[..., 0] + run[..., 1]
  acc = np.zeros(pair.shape[:-1], np.float32)
  for j in range(pair.shape[-1]):
    acc = acc + pair[..., j]
  return acc


def _tile_scale(ds, axis):
  """pow2_scale_of the maximum |ds| of each 64-wide tile of `axis` of [G, T, T']: per element of `axis`, [G, T]."""
  m = np.abs(ds).max(3 - axis)
  out = np.empty_like(m)
  for g in range(m.shape[0]):
    for n0 in range(0, m.shape[1], 64):
      out[g, n0:n0 + 64] = pow2_scale_of(m[g, n0:n0 + 64].max())
  return out


def model(q, k, v, do, heads, scale, betas=(0.0, 0.0, 0.0), g0=None, mutant=None):
  """The arithmetic of attention.hip on float32 [B, C, T] arrays (module text) -> the six outputs, float32.  mutant: one of
  'mask admits T', 'last 4 keys dropped', 'lse of the neighbouring head', 'delta of the neighbouring head',
  'head offset with C', 'hi lo dropped', 'ds scale of the image', 'beta_k and beta_v exchanged'."""
  with np.errstate(over='ignore', invalid='ignore'):           # a mutant may overflow: its result is then not finite
    return _model(q, k, v, do, heads, scale, betas, g0, mutant)


def _model(q, k, v, do, heads, scale, betas, g0, mutant):
  B, C, T = q.shape
  d = C // heads
  f32 = np.float32
  sc = {n: pow2_scale_of(np.abs(t).max()) for n, t in (('q', q), ('k', k), ('v', v), ('do', do))}

  def hv(x):                                               # [G, d, T], G = B heads
    x = heads_view(np.asarray(x, f32), heads)
    if mutant == 'head offset with C':                     # head n of image b read C T floats a head on: (b + n, head 0)
      y = np.zeros_like(x)
      for b in range(B):
        for n in range(heads):
          if b + n < B:
            y[b, n] = x[b + n, 0]
      x = y
    return np.ascontiguousarray(x.reshape(B * heads, d, T))

  q, k, v, do = hv(q), hv(k), hv(v), hv(do)
  live = T - 4 if mutant == 'last 4 keys dropped' else T
  if mutant == 'mask admits T':                            # one more key column, of zeros (what the loads return past T)
    k, v = (np.concatenate([t, np.zeros_like(t[:, :, :1])], 2) for t in (k, v))
    live = T + 1
  drop = mutant == 'hi lo dropped'
  t_ = lambda x: np.ascontiguousarray(x.transpose(0, 2, 1))
  qs, ks, vs, dos = _split(q, sc['q']), _split(k, sc['k']), _split(v, sc['v']), _split(do, sc['do'])
  us = f32(scale) / f32(sc['q'] * sc['k'])
  s = (us * _contract(qs, ks, drop))[:, :, :live]          # [G, t, t']
  # forward
  mx = s.max(-1)
  pf = np.exp(s - mx[..., None])
  sm = _reduce(pf)
  lse = (mx + np.log(sm)).astype(f32)
  pT = tuple(t_(x) for x in _split(pf, P_SCALE))           # [G, t', t]
  vT = tuple(t_(x[:, :, :live]) for x in vs)               # [G, t', c]
  o = (f32(1.0 / (sc['v'] * P_SCALE)) * (f32(1) / sm))[:, None, :] * _contract(vT, pT, drop)
  if mutant == 'mask admits T':                            # the backward's pad column has k = 0 and dp = 0: nothing to add
    k, v, live = k[:, :, :T], v[:, :, :T], T
    ks, vs, s = tuple(x[:, :, :T] for x in ks), tuple(x[:, :, :T] for x in vs), s[:, :, :T]
  # backward
  nb = lambda x: np.roll(x.reshape(B, heads, T), 1, 1).reshape(B * heads, T)
  lse_b = nb(lse) if mutant == 'lse of the neighbouring head' else lse
  pb = np.exp(s - lse_b[..., None]).astype(f32)
  dp = (f32(1.0 / (sc['do'] * sc['v'])) * _contract(dos, vs, drop))[:, :, :live]
  delta = _reduce(pb * dp)
  de = nb(delta) if mutant == 'delta of the neighbouring head' else delta
  ds = f32(scale) * (pb * (dp - de[..., None]))
  if mutant == 'ds scale of the image':
    img = np.array([pow2_scale_of(np.abs(ds[g]).max()) for g in range(ds.shape[0])])
    sq_, sk_ = np.repeat(img[:, None], ds.shape[1], 1), np.repeat(img[:, None], ds.shape[2], 1)
  else:
    sq_, sk_ = _tile_scale(ds, 1), _tile_scale(ds, 2)
  kT = tuple(t_(x[:, :, :live]) for x in ks)
  dsq = tuple(t_(x) for x in _split(ds, sq_[:, :, None]))                       # [G, t', t]
  dq = _contract(kT, dsq, drop) * (f32(1.0 / sc['k']) / sq_.astype(f32))[:, None, :]
  qT, doT = tuple(t_(x) for x in qs), tuple(t_(x) for x in dos)
  dk = _contract(qT, _split(ds, sk_[:, None, :]), drop) * (f32(1.0 / sc['q']) / sk_.astype(f32))[:, None, :]
  dv = _contract(doT, _split(pb, P_SCALE), drop) * f32(1.0 / (sc['do'] * P_SCALE))
  if live < T:                                             # the dropped keys get nothing
    pad = lambda x: np.concatenate([x, np.zeros(x.shape[:2] + (T - live,), f32)], 2)
    dk, dv = pad(dk), pad(dv)
  out = {'o': o, 'dq': dq, 'dk': dk, 'dv': dv}
  out = {n: t.astype(f32).reshape(B, C, T) for n, t in out.items()}
  bq, bk, bv = betas
  if mutant == 'beta_k and beta_v exchanged':
    bk, bv = bv, bk
  for n, beta, i in (('dq', bq, 0), ('dk', bk, 1), ('dv', bv, 2)):
    if beta != 0.0:
      out[n] = (np.float64(beta) * np.asarray(g0[i], np.float64) + out[n].astype(np.float64)).astype(f32)
  out['lse'], out['delta'] = lse.reshape(B, heads, T), delta.reshape(B, heads, T)
  return out
