"""Float64 restatements of the entries of csrc/elementwise.hip, and the bound each element is held to.

Every function takes the parameters p (a dict) and the float32 operands a (a dict of numpy arrays) of one case of
tests/_ew_cases.py and returns Ref(want, B, k[, floor]) -- or a dict of them, one per output:

  want   the exact result, computed in float64 from the float32 operands (and from the float32 values of the scalar
         arguments: what the C ABI receives)
  B      the magnitude of that element: the same expression on absolute values
  k      the unit count: |got - want| <= k u B + floor, u = 2^-24
  floor  2^-126, so that a flushed subnormal is no error; larger only where an INTERMEDIATE underflows and is scaled
         afterwards: SiLU below x = -87.34, by the term that is lost (_sigmoid_floor)
  k = 0  means: compared bit for bit with want (a float32 / uint8 array)

How k is counted.  A correctly rounded +, -, *, / or fma is off by at most u of the magnitude of its own result (HIP's
default float32 division is correctly rounded; a contracted fma only removes a rounding, so the uncontracted sequence is
counted).  expf / expm1f are charged 3 ulp = 6 u of |result|, sinf / cosf 4 ulp = 8 u of |result| <= 8 u absolute (the
OpenCL full-profile limits OCML is built to meet).  An error in an argument goes through the derivative: an argument of
sin / cos built with `a` roundings is off by a u |arg|, absolute, and so is the result.  One more unit covers the
second-order terms.  No figure here was measured on a kernel; tests/test_ew_cases_cpu.py shows that the plain-C checker
and a float32 numpy restatement (the *_f32 functions below, same signature, returning the arrays) meet every one.
"""
import collections
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
Ref = collections.namedtuple('Ref', 'want B k floor', defaults=(TINY,))
PI_F = float(np.float32(math.pi))          # 3.14159274101257324f
F = np.float32


def f32(v):
  """The float32 value a float argument of the C ABI arrives as."""
  return float(np.float32(v))


def _d(x):
  return np.asarray(x, dtype=np.float64)


def _sigmoid(x):
  with np.errstate(over='ignore'):
    return 1.0 / (1.0 + np.exp(-x))


def depth(length):
  """Roundings on the longest path of block_sum over `length` terms: ceil(length / 256) serial steps of a lane, 6 shuffle
  steps of a wave of 64, 4 wave partials."""
  return -(-length // 256) + 6 + 4


# ---- activations ----------------------------------------------------------------------------------------------------
def _act_value(act, x):
  """-> (want, k).  SiLU x / (1 + e), e = expf(-x): e is off by 6 u e, d = 1 + e by 6 u e + u d = (6 (1 - s) + 1) u d with
  s = 1 / d the sigmoid, the quotient rounds once: (8 - 6 s) u <= 8 u of |y|, and one unit more: k = 9.  LeakyReLU: one
  product, k = 2.  ELU below 0: expm1f, k = 6 + 1 = 7.  Identity and ReLU: no arithmetic, bit for bit."""
  with np.errstate(over='ignore'):
    if act == 1:
      return x * _sigmoid(x), 9
    if act == 2:
      return np.where(x > 0, x, 0.0), 0
    if act == 3:
      return np.where(x > 0, x, _d(F(0.2)) * x), 2
    if act == 4:
      return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0))), 7
  return x, 0


def _act_slope(act, x):
  """-> (slope, S, kg): the slope, its magnitude on absolute values and the units of |dy| S that g = dy * slope is off by.

  SiLU: sg = 1 / (1 + e) carries (8 - 6 s) u sg (see _act_value); om = 1 - sg, t = x om, w = 1 + t and the products sg w
  and dy (sg w) round once each.  With S = s (1 + |x|), in units of u |dy| s:
    the error of sg, through d/dsg [sg (1 + x (1 - sg))] = 1 + x (1 - 2 s):    (8 - 6 s) |1 + x (1 - 2 s)|
    the roundings of om and t:                                                  2 |x| (1 - s)
    the rounding of w and the two products:                                     3 |1 + x (1 - s)|
  Their sum over 1 + |x| rises to 13 as x -> -inf (8 + 2 + 3) and stays below it everywhere else (2 as x -> +inf, 6.1 at
  x = -3, 10.8 at x = -10): kg = 13.  The other slopes are constants (1, 0, 0.2f): the product rounds once, kg = 1; ELU
  below 0 is expf: kg = 6 + 1 = 7."""
  ax = np.abs(x)
  if act == 1:
    s = _sigmoid(x)
    return s * (1.0 + x * (1.0 - s)), s * (1.0 + ax), 13
  if act == 2:
    sl = np.where(x > 0, 1.0, 0.0)
    return sl, sl, 1
  if act == 3:
    sl = np.where(x > 0, 1.0, _d(F(0.2)))
    return sl, sl, 1
  if act == 4:
    with np.errstate(over='ignore'):
      sl = np.where(x > 0, 1.0, np.exp(np.minimum(x, 0.0)))
    return sl, sl, 7
  return np.ones_like(x), np.ones_like(x), 1


SIGMOID_UNDERFLOWS = -126.0 * math.log(2.0)                     # x < -87.34: the sigmoid is below 2^-126


def _sigmoid_floor(x, term):
  """The floor of a SiLU entry, `term` being the exact value of what its sigmoid s multiplies into (x s forward, dy times
  the slope backward).  Below x = -126 ln 2 = -87.34, s < 2^-126: the float32 s is a subnormal, which correct float32
  arithmetic either keeps (then the error is relative and k u B covers it) or flushes to 0 -- and it IS 0 below -88.72,
  where e^-x leaves the float32 range and the forward quotient is -0.  A flushed s loses the whole term, up to 2e-37 at
  x = -89, so there the floor is 2^-126 + |term|: zero is accepted, a value further from `term` than `term` itself is
  not.  At -1e4 and -3e38 the term is 0 and the floor is the plain 2^-126, as it is everywhere above -87.34."""
  return np.where(x < SIGMOID_UNDERFLOWS, TINY + np.abs(term), TINY)


def act_fwd(p, a):
  """See _act_value; the floor of SiLU is _sigmoid_floor's, the term being the result itself."""
  x = _d(a['x'])
  want, k = _act_value(p['act'], x)
  if k == 0:
    return Ref(want.astype(np.float32), None, 0)
  return Ref(want, np.abs(want), k, _sigmoid_floor(x, want) if p['act'] == 1 else TINY)


def act_bwd(p, a):
  """dx = beta dx0 + dy slope(x), B = |dy| S + |beta dx0| (SiLU: S = s (1 + |x|): 1 + x (1 - s) cancels near x = -1.28, and
  for large x, 1 - s carries an absolute u / 2).  k = kg (see _act_slope) + the product beta dx0 + the sum + 1 = kg + 3;
  beta = 0 skips the product and the sum is exact: k = kg + 1.  SiLU: 16 and 14, and the floor is
  _sigmoid_floor's, the term being dy slope(x)."""
  x, dy, beta = _d(a['x']), _d(a['dy']), p['beta']
  sl, S, kg = _act_slope(p['act'], x)
  want, B = dy * sl, np.abs(dy) * S
  floor = _sigmoid_floor(x, want) if p['act'] == 1 else TINY
  if beta != 0.0:
    want, B = want + beta * _d(a['dx0']), B + np.abs(beta * _d(a['dx0']))
  return Ref(want, B, kg + (3 if beta != 0.0 else 1), floor)


silu_fwd = lambda p, a: act_fwd(dict(p, act=1), a)
silu_bwd = lambda p, a: act_bwd(dict(p, act=1), a)


def _act_value_f32(act, x):
  with np.errstate(over='ignore', under='ignore'):
    if act == 1:
      return x / (F(1) + np.exp(-x))
    if act == 2:
      return np.where(x > 0, x, F(0))
    if act == 3:
      return np.where(x > 0, x, F(0.2) * x)
    if act == 4:
      return np.where(x > 0, x, np.expm1(np.minimum(x, F(0))))
  return x.copy()


def act_fwd_f32(p, a):
  return _act_value_f32(p['act'], a['x'])


def act_bwd_f32(p, a):
  x, dy, act, beta = a['x'], a['dy'], p['act'], F(p['beta'])
  with np.errstate(over='ignore', under='ignore'):
    if act == 1:
      sg = F(1) / (F(1) + np.exp(-x))
      sl = sg * (F(1) + x * (F(1) - sg))
    elif act == 2:
      sl = np.where(x > 0, F(1), F(0))
    elif act == 3:
      sl = np.where(x > 0, F(1), F(0.2))
    elif act == 4:
      sl = np.where(x > 0, F(1), np.exp(np.minimum(x, F(0))))
    else:
      sl = np.ones_like(x)
    g = dy * sl
    return g if beta == 0 else beta * a['dx0'] + g


silu_fwd_f32 = lambda p, a: act_fwd_f32(dict(p, act=1), a)
silu_bwd_f32 = lambda p, a: act_bwd_f32(dict(p, act=1), a)


# ---- flat arithmetic ------------------------------------------------------------------------------------------------
def axpby(p, a):
  """alpha a + beta b, B = |alpha a| + |beta b|: two products, one sum, one unit more: k = 4.  b absent or beta = 0 (b is
  not read then): one product, k = 2."""
  x, alpha, beta = _d(a['a']), p['alpha'], p['beta']
  if a.get('b') is None or beta == 0.0:
    return Ref(alpha * x, np.abs(alpha * x), 2)
  y = _d(a['b'])
  return Ref(alpha * x + beta * y, np.abs(alpha * x) + np.abs(beta * y), 4)


def axpby_f32(p, a):
  if a.get('b') is None or p['beta'] == 0.0:
    return F(p['alpha']) * a['a']
  return F(p['alpha']) * a['a'] + F(p['beta']) * a['b']


def add_div(p, a):
  """(a + b) / div, B = (|a| + |b|) / |div|: the sum, the host's float32 1 / div and the product round once each, one more:
  k = 4; div = 1 is the sum alone, k = 2."""
  s, B = _d(a['a']) + _d(a['b']), np.abs(_d(a['a'])) + np.abs(_d(a['b']))
  return Ref(s / p['div'], B / abs(p['div']), 2 if p['div'] == 1.0 else 4)


def add_div_f32(p, a):
  s = a['a'] + a['b']
  return s if p['div'] == 1.0 else s * (F(1) / F(p['div']))


def affine(p, a):
  """a x + b, B = |a x| + |b|: a product and a sum, one more: k = 3."""
  ax = p['a'] * _d(a['x'])
  return Ref(ax + p['b'], np.abs(ax) + abs(p['b']), 3)


def affine_f32(p, a):
  return F(p['a']) * a['x'] + F(p['b'])


def fill(p, a):
  """No arithmetic: bit for bit."""
  return Ref(np.full(p['n'], p['v'], dtype=np.float32), None, 0)


fill_f32 = lambda p, a: fill(p, a).want


def fill_strided(p, a):
  """No arithmetic: bit for bit, the gaps between the runs keep what they held."""
  out = a['out0'].copy()
  for i in range(p['count']):
    out[i * p['stride']:i * p['stride'] + p['len']] = p['v']
  return Ref(out, None, 0)


fill_strided_f32 = lambda p, a: fill_strided(p, a).want


def _bias_act(p, a, dt):
  x = a['x'].astype(dt)
  n = x.size
  t, T = x, np.abs(x)
  if a.get('b') is not None:
    bb = a['b'].astype(dt)[(np.arange(n) // p['step_b']) % p['size_b']]
    t, T = x + bb, T + np.abs(bb)
  alpha, scale, code = dt(p['alpha']), dt(p['scale']), p['act'] * 10 + p['grad']
  rr = a['ref'].astype(dt) if a.get('ref') is not None else np.zeros(n, dt)
  if code in (12, 32):
    y, Y = np.zeros(n, dt), np.zeros(n, dt)
  elif code == 30:
    y, Y = np.where(t > 0, t, t * alpha), np.where(t > 0, T, T * abs(alpha))
  elif code == 31:
    y, Y = np.where(rr > 0, t, t * alpha), np.where(rr > 0, T, T * abs(alpha))
  else:
    y, Y = t, T
  return y * scale, Y * abs(scale)


def fused_bias_act(p, a):
  """((x + b) [alpha]) scale, B the same on absolute values: the sum, the slope and the gain round once each, one more:
  k = 4.  The sign test is exact: a rounded sum has the sign of the exact one.  f64: the same count in units of 2^-53.
  f16: computed in float32 and rounded to half once: 2^-11 |want| + 4 u B + 2^-25 (tests/_ew_cases.py applies it)."""
  want, B = _bias_act(p, a, np.float64)
  return Ref(want, B, 4)


def fused_bias_act_f32(p, a):
  return _bias_act(p, a, np.float32)[0]


# ---- row-indexed ----------------------------------------------------------------------------------------------------
def _rows(v, inner):
  return np.repeat(_d(v), inner)


def rowscale(p, a):
  """x s[n] or x / s[n]: one rounding, one more: k = 2, B = |want|."""
  s = _rows(a['s'], p['inner'])
  want = _d(a['x']) * s if p['mode'] == 0 else _d(a['x']) / s
  return Ref(want, np.abs(want), 2)


def rowscale_f32(p, a):
  s = np.repeat(a['s'], p['inner'])
  return a['x'] * s if p['mode'] == 0 else a['x'] / s


def perturb(p, a):
  """a[n] x + s[n] z: two products and a sum, one more: k = 4; without a: k = 3.  B on absolute values."""
  sz = _rows(a['s'], p['inner']) * _d(a['z'])
  if a.get('a') is None:
    return Ref(_d(a['x']) + sz, np.abs(_d(a['x'])) + np.abs(sz), 3)
  ax = _rows(a['a'], p['inner']) * _d(a['x'])
  return Ref(ax + sz, np.abs(ax) + np.abs(sz), 4)


def perturb_f32(p, a):
  sz = np.repeat(a['s'], p['inner']) * a['z']
  return (a['x'] if a.get('a') is None else np.repeat(a['a'], p['inner']) * a['x']) + sz


def _residual(p, o, z, sd):
  """r of losses.py:122-132 in float64 -> (r, R, units): R on absolute values, the error of the float32 r <= units u R.
  vp: score = -o / sd rounds once (|o| / sd).  mode 0: r = score sd + z, the product and the sum round once each and
  R = |o| + |z|; mode 1: r = score + z / sd, the quotient and the sum, R = |score| + |z| / sd.  units = vp + 2."""
  score, S = (-o / sd, np.abs(o) / sd) if p['vp'] else (o, np.abs(o))
  if p['mode'] == 0:
    return score * sd + z, S * sd + np.abs(z), p['vp'] + 2
  return score + z / sd, S + np.abs(z) / sd, p['vp'] + 2


def sm_loss_bwd(p, a):
  """dnet = [-1 / sd] c r [sd], c = 2 dloss wgt red, red = 1 / inner or 1 / 2; B the chain on absolute values.
  c: two products, and the float32 1 / inner when reduce_mean (the factor 2 and 1 / 2 are exact): 2 + rm; r: vp + 2 (see
  _residual); c r [sd]: 2 - mode products; the final quotient when vp: vp; one more:
  k = (2 + rm) + (vp + 2) + (2 - mode) + vp + 1, from 6 (VE, mode 1, sum) to 10 (VP, mode 0, mean)."""
  inner, vp, mode, rm = p['inner'], p['vp'], p['mode'], p['rm']
  sd = _rows(a['std'], inner)
  r, Rm, ur = _residual(p, _d(a['net']), _d(a['z']), sd)
  c = _rows(a['dloss'], inner) * _rows(a['wgt'], inner) * (2.0 / inner if rm else 1.0)
  want, B = c * r, np.abs(c) * Rm
  if mode == 0:
    want, B = want * sd, B * sd
  if vp:
    want, B = -want / sd, B / sd
  return Ref(want, B, (2 + rm) + ur + (2 - mode) + vp + 1)


def _residual_f32(p, o, z, sd):
  score = -o / sd if p['vp'] else o
  return score * sd + z if p['mode'] == 0 else score + z / sd


def sm_loss_bwd_f32(p, a):
  inner = p['inner']
  sd = np.repeat(a['std'], inner)
  r = _residual_f32(p, a['net'], a['z'], sd)
  red = F(1) / F(inner) if p['rm'] else F(0.5)
  c = np.repeat(a['dloss'] * a['wgt'] * red * F(2), inner)
  gs = c * r * sd if p['mode'] == 0 else c * r
  return -gs / sd if p['vp'] else gs


def sm_loss_fwd(p, a):
  """loss[n] = wgt red sum_i r_i^2, B = wgt red sum_i R_i^2 with R the chain of r on absolute values (sum r^2 itself would
  not bound a residual that cancels).  r is off by (vp + 2) u R, r^2 by twice that and its own rounding: 2 vp + 5 units of
  R^2; the sum adds depth(inner) roundings of partial sums that sum R^2 bounds; the mean divides (rm), wgt multiplies (1),
  one more: k = 2 vp + 5 + depth(inner) + rm + 2."""
  N, inner = p['N'], p['inner']
  sd = _rows(a['std'], inner)
  r, Rm, _ = _residual(p, _d(a['net']), _d(a['z']), sd)
  red = 1.0 / inner if p['rm'] else 0.5
  w = _d(a['wgt']) * red
  return Ref(w * (r * r).reshape(N, inner).sum(1), w * (Rm * Rm).reshape(N, inner).sum(1),
             2 * p['vp'] + 5 + depth(inner) + p['rm'] + 2)


def sm_loss_fwd_f32(p, a):
  N, inner = p['N'], p['inner']
  r = _residual_f32(p, a['net'], a['z'], np.repeat(a['std'], inner))
  s = np.sum((r * r).reshape(N, inner), axis=1, dtype=np.float32)
  return a['wgt'] * (s / F(inner) if p['rm'] else F(0.5) * s)


# ---- embeddings -----------------------------------------------------------------------------------------------------
def _trig(arg, a_units, argmax):
  """sin / cos of an argument built with a_units roundings: |error| <= (a_units |arg| + 8 + 1) u.  The case states
  argmax >= |arg|; k = a_units argmax + 9 and B = (a_units |arg| + 9) / k <= 1 is the element's share of it."""
  assert float(np.abs(arg).max()) <= argmax, (float(np.abs(arg).max()), argmax)
  k = a_units * argmax + 9
  return k, (a_units * np.abs(arg) + 9.0) / k


def timestep_embedding(p, a):
  """out[b] = [sin(t f), cos(t f), 0 if dim is odd]: the argument is one float32 product of two float32 operands, a = 1;
  |arg| <= p['argmax'] (t <= 999, f <= 1: about 1000 rad).  The zero column is exactly 0: its B is 0."""
  B_, dim, half = p['B'], p['dim'], p['dim'] // 2
  arg = _d(a['t'])[:, None] * _d(a['freqs'])[None, :]
  k, share = _trig(arg, 1, p['argmax'])
  want, mag = np.zeros((B_, dim)), np.zeros((B_, dim))
  want[:, :half], want[:, half:2 * half] = np.sin(arg), np.cos(arg)
  mag[:, :half], mag[:, half:2 * half] = share, share
  return Ref(want, mag, k, np.where(mag > 0, TINY, 0.0))


def timestep_embedding_f32(p, a):
  half = p['dim'] // 2
  arg = a['t'][:, None] * a['freqs'][None, :]
  out = np.zeros((p['B'], p['dim']), np.float32)
  out[:, :half], out[:, half:2 * half] = np.sin(arg), np.cos(arg)
  return out


def fourier_embedding(p, a):
  """[sin(2 pi x W), cos(2 pi x W)]: x W rounds, the factor 2 is exact, the float32 pi differs from pi (0.47 u, charged 1)
  and its product rounds: a = 3; |arg| <= p['argmax'] (about 2000 rad at |x| <= 5.9, |W| <= 56)."""
  arg = _d(a['x'])[:, None] * _d(a['W'])[None, :] * (2.0 * math.pi)
  k, share = _trig(arg, 3, p['argmax'])
  return Ref(np.concatenate([np.sin(arg), np.cos(arg)], 1), np.concatenate([share, share], 1), k)


def fourier_embedding_f32(p, a):
  arg = a['x'][:, None] * a['W'][None, :] * F(2) * F(math.pi)
  return np.concatenate([np.sin(arg), np.cos(arg)], 1)


def fourier_embedding_bwd(p, a):
  """dx[b] = beta dx0[b] + 2 pi sum_j W_j (g_j c_j - g_{nf+j} s_j), c / s the float32 forward output handed in as y: no
  trigonometric function enters.  B = 2 pi sum |W_j| (|g_j c_j| + |g_{nf+j} s_j|) + |beta dx0|.  Per term: the two
  products (one unit of their own sum), the difference, the product with W: 3; the sum: depth(nf); the float32 2 pi
  (charged 1) and its product: 2; beta dx0 and the final sum: 2 (absent at beta = 0); one more."""
  nf, beta = p['nf'], p['beta']
  W, y, g = _d(a['W'])[None, :], _d(a['y']), _d(a['dy'])
  gc, gs = g[:, :nf] * y[:, nf:], g[:, nf:] * y[:, :nf]
  want = 2.0 * math.pi * (W * (gc - gs)).sum(1)
  B = 2.0 * math.pi * (np.abs(W) * (np.abs(gc) + np.abs(gs))).sum(1)
  k = 3 + depth(nf) + 2 + 1
  if beta != 0.0:
    want, B, k = want + beta * _d(a['dx0']), B + np.abs(beta * _d(a['dx0'])), k + 2
  return Ref(want, B, k)


def fourier_embedding_bwd_f32(p, a):
  nf, W, y, g = p['nf'], a['W'][None, :], a['y'], a['dy']
  acc = np.sum(W * (g[:, :nf] * y[:, nf:] - g[:, nf:] * y[:, :nf]), axis=1, dtype=np.float32)
  out = F(2) * F(math.pi) * acc
  return out if p['beta'] == 0.0 else F(p['beta']) * a['dx0'] + out


def fixed_fourier_fwd(p, a):
  """[x, sin(128 pi x), cos(128 pi x), sin(256 pi x), cos(256 pi x)] along the channels.  128 x is exact, the float32 pi and
  its product: a = 2; |arg| <= 256 pi |x| <= p['argmax'] (804.3 rad at |x| = 1).  The copy of x is bit for bit (B = 0)."""
  N, C, HW = p['N'], p['C'], p['HW']
  x = _d(a['x']).reshape(N, C * HW)
  a1, a2 = 128.0 * math.pi * x, 256.0 * math.pi * x
  k, s1 = _trig(a1, 2, p['argmax'])
  _, s2 = _trig(a2, 2, p['argmax'])
  want = np.stack([x, np.sin(a1), np.cos(a1), np.sin(a2), np.cos(a2)], 1)
  mag = np.stack([np.zeros_like(x), s1, s1, s2, s2], 1)
  return Ref(want, mag, k, np.where(mag > 0, TINY, 0.0))


def fixed_fourier_fwd_f32(p, a):
  x = a['x'].reshape(p['N'], p['C'] * p['HW'])
  a1, a2 = (x * F(128)) * F(PI_F), (x * F(256)) * F(PI_F)
  return np.stack([x, np.sin(a1), np.cos(a1), np.sin(a2), np.cos(a2)], 1)


def fixed_fourier_bwd(p, a):
  """dx = beta dx0 + d0 + 128 pi (c1 d1 - s1 d2) + 256 pi (c2 d3 - s2 d4).  With T1 = 128 pi (|d1| + |d2|), T2 = 256 pi
  (|d3| + |d4|) (|c|, |s| set to 1) and M = |beta dx0| + |d0| + T1 + T2: the sines and cosines are off by (2 |arg| + 8) u
  absolute (fixed_fourier_fwd), which T1 and T2 scale; on top, in units of M: the two products and the difference (2), the
  float32 128 pi (1) and its product (1), the two sums (2), beta dx0 and its sum (2), one more (1).  So
  |error| <= u [9 M + (2 |a1| + 8) T1 + (2 |a2| + 8) T2]; stated as k = 2 argmax + 8 + 9 with B that bracket over k (<= M)."""
  N, C, HW, beta = p['N'], p['C'], p['HW'], p['beta']
  x = _d(a['x']).reshape(N, C * HW)
  d = _d(a['dy']).reshape(N, 5, C * HW)
  a1, a2 = 128.0 * math.pi * x, 256.0 * math.pi * x
  assert float(np.abs(a2).max()) <= p['argmax']
  want = d[:, 0] + 128.0 * math.pi * (np.cos(a1) * d[:, 1] - np.sin(a1) * d[:, 2]) \
      + 256.0 * math.pi * (np.cos(a2) * d[:, 3] - np.sin(a2) * d[:, 4])
  T1, T2 = 128.0 * math.pi * (np.abs(d[:, 1]) + np.abs(d[:, 2])), 256.0 * math.pi * (np.abs(d[:, 3]) + np.abs(d[:, 4]))
  M = np.abs(d[:, 0]) + T1 + T2
  if beta != 0.0:
    dx0 = _d(a['dx0']).reshape(N, C * HW)
    want, M = want + beta * dx0, M + np.abs(beta * dx0)
  k = 2 * p['argmax'] + 8 + 9
  return Ref(want, (9.0 * M + (2.0 * np.abs(a1) + 8.0) * T1 + (2.0 * np.abs(a2) + 8.0) * T2) / k, k)


def fixed_fourier_bwd_f32(p, a):
  N, C, HW = p['N'], p['C'], p['HW']
  x, d = a['x'].reshape(N, C * HW), a['dy'].reshape(N, 5, C * HW)
  a1, a2 = (x * F(128)) * F(PI_F), (x * F(256)) * F(PI_F)
  g = d[:, 0] + (F(128) * F(PI_F)) * (np.cos(a1) * d[:, 1] - np.sin(a1) * d[:, 2]) \
      + (F(256) * F(PI_F)) * (np.cos(a2) * d[:, 3] - np.sin(a2) * d[:, 4])
  return g if p['beta'] == 0.0 else F(p['beta']) * a['dx0'].reshape(N, C * HW) + g


# ---- data movement --------------------------------------------------------------------------------------------------
def concat(p, a):
  """torch.cat along the channels: no arithmetic, bit for bit."""
  N, Ca, Cb, HW = p['N'], p['Ca'], p['Cb'], p['HW']
  return Ref(np.concatenate([a['a'].reshape(N, Ca * HW), a['b'].reshape(N, Cb * HW)], 1), None, 0)


concat_f32 = lambda p, a: concat(p, a).want


def concat_bwd(p, a):
  """da = beta da0 + dout[:, :Ca], db likewise.  beta = 0: a copy, bit for bit; else the product and the sum, one more:
  k = 3, B = |beta d0| + |g|."""
  N, Ca, Cb, HW, beta = p['N'], p['Ca'], p['Cb'], p['HW'], p['beta']
  g = a['dout'].reshape(N, (Ca + Cb) * HW)
  out = {}
  for name, part in (('da', g[:, :Ca * HW]), ('db', g[:, Ca * HW:])):
    if beta == 0.0:
      out[name] = Ref(np.ascontiguousarray(part), None, 0)
    else:
      old = beta * _d(a[name + '0']).reshape(part.shape)
      out[name] = Ref(old + _d(part), np.abs(old) + np.abs(_d(part)), 3)
  return out


def concat_bwd_f32(p, a):
  N, Ca, Cb, HW, beta = p['N'], p['Ca'], p['Cb'], p['HW'], p['beta']
  g = a['dout'].reshape(N, (Ca + Cb) * HW)
  out = {'da': np.ascontiguousarray(g[:, :Ca * HW]), 'db': np.ascontiguousarray(g[:, Ca * HW:])}
  if beta != 0.0:
    out = {n: F(beta) * a[n + '0'].reshape(v.shape) + v for n, v in out.items()}
  return out


def resample_naive(p, a):
  """up: out = beta out0 + alpha in[y / 2, x / 2]: two products and a sum, one more: k = 4 (beta = 0: k = 2).
  down: out = beta out0 + alpha ((a + b) + (c + d)) / 4: three sums, each within u of the sum of absolute values (the
  quarter is exact), then as before: k = 7 (beta = 0: k = 5).  B on absolute values."""
  P, H, W, alpha, beta = p['planes'], p['H'], p['W'], p['alpha'], p['beta']
  x = _d(a['in']).reshape(P, H, W)
  if p['mode'] == 0:
    want = alpha * x.repeat(2, 1).repeat(2, 2)
    B, k = np.abs(want), 2
  else:
    q = x.reshape(P, H // 2, 2, W // 2, 2)
    want, B, k = alpha * q.sum((2, 4)) / 4.0, abs(alpha) * np.abs(q).sum((2, 4)) / 4.0, 5
  if beta != 0.0:
    old = beta * _d(a['out0']).reshape(want.shape)
    want, B, k = want + old, B + np.abs(old), k + 2
  return Ref(want, B, k)


def resample_naive_f32(p, a):
  P, H, W = p['planes'], p['H'], p['W']
  x = a['in'].reshape(P, H, W)
  if p['mode'] == 0:
    m = x.repeat(2, 1).repeat(2, 2)
  else:
    q = x.reshape(P, H // 2, 2, W // 2, 2)
    m = ((q[:, :, 0, :, 0] + q[:, :, 0, :, 1]) + (q[:, :, 1, :, 0] + q[:, :, 1, :, 1])) * F(0.25)
  out = F(p['alpha']) * m
  return out if p['beta'] == 0.0 else F(p['beta']) * a['out0'].reshape(out.shape) + out


# ---- the shared counter RNG (include/stk_rng.h) and what is drawn from it ----------------------------------------------
def mix64(seed, i):
  with np.errstate(over='ignore'):
    z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.asarray(i, np.uint64) + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
  return z ^ (z >> np.uint64(31))


def uniform(seed, i):
  i = np.asarray(i, np.uint64)
  z = mix64(seed, i >> np.uint64(1))
  bits = np.where(i & np.uint64(1), (z >> np.uint64(8)) & np.uint64(0xFFFFFF), z >> np.uint64(40))
  return bits.astype(np.float32) * F(1.0 / 16777216.0)


def dropout_mask(p, a):
  """mask[i] = keep(seed, i) ? 1 / (1 - p) : 0 with the float32 quotient: the draw is integer arithmetic, bit for bit."""
  i = np.arange(p['n'], dtype=np.uint64)
  thr = np.uint64(int(F(p['p']) * F(65536.0) + F(0.5)))
  field = (mix64(p['seed'], i >> np.uint64(2)) >> (np.uint64(16) * (i & np.uint64(3)))) & np.uint64(0xFFFF)
  return Ref(np.where(field >= thr, F(1) / (F(1) - F(p['p'])), F(0)).astype(np.float32), None, 0)


dropout_mask_f32 = lambda p, a: dropout_mask(p, a).want


def samples_to_uint8(p, a):
  """uint8(clip(255 x, 0, 255)), NCHW -> NHWC: the float32 numpy expression, bit for bit."""
  x = a['x'].reshape(p['N'], p['C'], p['HW'])
  return Ref(np.clip(x * F(255), 0, 255).astype(np.uint8).transpose(0, 2, 1).copy(), None, 0)


samples_to_uint8_f32 = lambda p, a: samples_to_uint8(p, a).want


def preprocess_u8(p, a):
  """u8 NHWC -> float NCHW, v = u8 (1 / 255.f), mirrored per image by the shared draw, [2 v - 1].  dequant = 0: the float32
  numpy expression bit for bit (2 v is exact, so a contracted 2 v - 1 rounds the same).  dequant = 1: `want` is the
  dequant = 0 value BEFORE centring; tests/_ew_cases.py checks the interval [255 v, 255 v + 1] / 256 around it."""
  N, C, H, W = p['N'], p['C'], p['H'], p['W']
  img = a['img'].reshape(N, H, W, C)
  if p['flip']:
    f = uniform(p['seed'] ^ 0x5DEECE66D, np.arange(N)) < F(0.5)
    img = np.where(f[:, None, None, None], img[:, :, ::-1, :], img)
  v = img.transpose(0, 3, 1, 2).astype(np.float32) * F(1.0 / 255.0)
  if p['centered'] and not p['dequant']:
    v = v * F(2) - F(1)
  return Ref(np.ascontiguousarray(v), None, 0)


def preprocess_u8_f32(p, a):
  v = preprocess_u8(p, a).want
  if p['dequant']:
    v = (F(255) * v + uniform(p['seed'], np.arange(v.size)).reshape(v.shape)) * F(1.0 / 256.0)
    if p['centered']:
      v = v * F(2) - F(1)
  return v
