"""The geometric augmentation of include/stk_augment.h restated literally in numpy, and the bound its kernel is held to.

`warp` follows the definition step by step on ONE plane: flip, ``np.pad(.., 'reflect')`` by a margin computed from the case's
own matrix, zero-stuffing, full convolution with 2 f, bilinear gather at 2u - 1/2, convolution with f and decimation.  It knows
nothing of the periodic lattice of U that the kernel indexes through.  It reads the fp32 parameter row and taps the kernel
gets; in float64 (the reference) nothing is rounded, in float32 (`dtype=np.float32`, the check of the bound on the host)
every operation is, in the order the header states.

The bound, per output element:    gamma_n P(|S|; |f|)  +  D(L (delta_x + delta_y); |f|)

  gamma_n = n 2^-24 / (1 - n 2^-24), n = 3 T + 5: the roundings on the longest path of the kernel as written.  The up pass
      sums T/2 products per axis (the other taps meet zeros and are left out): a sum of m products carries m roundings on its
      first term (one product, m - 1 sums), the doubling is exact: T/2 + T/2.  The bilinear stage is
      (w00 U00 + w01 U01) + (w10 U10 + w11 U11) with w00 = (1 - gy)(1 - gx): 1 - g, the product of the two factors, the product
      with U and two sums: 5; g = s - floor(s) is exact.  The down pass sums T products per axis: T + T.  Every one is a
      relative error of a partial result whose magnitude the same pipeline run on |S| with taps |f| dominates (all weights
      there are non-negative, so no cancellation hides anything): that pipeline is P.
  delta: the fp32 error of the sampling coordinate s = 2u - 1/2, u = ((a dx + b dy) + c) + t'.  dx, dy (quarters below 2^8)
      and the reduced translation t' (fmodf and one Sterbenz subtraction) are exact.  Two products, then three sums, each
      rounded relative to a partial result of magnitude at most M = |a dx| + |b dy| + |c| + |t'|: at most 4 roundings meet any
      term, so |u_fp32 - u| <= gamma_4 M; doubling is exact and the last subtraction adds 2^-24 |s| <= 2^-24 (2 M + 1/2).
      delta = 2^-24 (10 M + 1) / (1 - 8 2^-24) covers both.  It follows the element: M is evaluated per point of the 2x grid.
  L: the largest difference between neighbouring values of U of that plane, along either axis (the extension of U beyond
      its 2H x 2W values only repeats them, and its mirror points repeat a value: no larger step exists).  Bilinear
      interpolation is continuous and piecewise linear with slopes bounded by those differences, so a coordinate error of
      (delta_x, delta_y) moves V by at most L (delta_x + delta_y) -- also when floor() lands on the other side of a lattice line.
  D(.; |f|): an error of V reaches an output element through the down pass, weighted by |f| along both axes; the bound
      sends the per-point term through that pass instead of taking one coordinate's delta for the whole window.
"""
import numpy as np

EPS = 2.0 ** -24


def default_filter():
  """The 12-tap Kaiser-windowed half-band sinc of the issue, in float64 then fp32."""
  k = np.arange(12, dtype=np.float64)
  f = np.sinc((k - 5.5) / 2.0) * np.kaiser(12, 8.0)
  return (f / f.sum()).astype(np.float32)


def box_filter(T):
  """T equal taps (T = 2: nearest-neighbour upsampling and a 2 x 2 mean)."""
  return np.full(T, 1.0 / T, dtype=np.float32)


def tent4():
  return np.array([0.125, 0.375, 0.375, 0.125], dtype=np.float32)


def row(fx=0, fy=0, G=None, shift=(0.0, 0.0)):
  """The fp32 parameter row of a FORWARD map: the image is transformed by the 2 x 2 matrix G about its centre and then
  shifted by `shift` pixels; the row holds the inverse, A = G^-1 and t = -A shift, built in float64 and rounded once."""
  G = np.eye(2) if G is None else np.asarray(G, dtype=np.float64)
  A = np.linalg.inv(G)
  t = -A @ np.asarray(shift, dtype=np.float64)
  return np.array([fx, fy, A[0, 0], A[0, 1], A[1, 0], A[1, 1], t[0], t[1]], dtype=np.float32)


def rot(deg):
  if deg % 90 == 0:
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][(deg // 90) % 4]
    return np.array([[c, -s], [s, c]], dtype=np.float64)
  a = np.deg2rad(deg)
  return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


def is_identity(p):
  return bool(p[2] == 1 and p[3] == 0 and p[4] == 0 and p[5] == 1 and p[6] == 0 and p[7] == 0)


def reduced_translation(t, n):
  """The kernel's exact reduction of a translation by whole periods 2(n-1) of U into [-(n-1), n-1], in fp32."""
  P, half = np.float32(2 * n - 2), np.float32(n - 1)
  r = np.fmod(np.float32(t), P)
  if r > half:
    r = np.float32(r - P)
  if r < -half:
    r = np.float32(r + P)
  return np.float32(r)


def _coords(p, H, W, T, dtype, reduce):
  """(sx, sy, Mx, My) on the (2H + T - 2) x (2W + T - 2) grid of V: the sampling coordinate 2u - 1/2 evaluated in `dtype` in
  the kernel's order, and the magnitude M of the bound."""
  h = T // 2
  t0, t1 = p[6], p[7]
  if reduce:
    t0, t1 = reduced_translation(t0, W), reduced_translation(t1, H)
  f = dtype
  qx = np.arange(-(h - 1), 2 * W + h - 1).astype(f)[None, :]
  qy = np.arange(-(h - 1), 2 * H + h - 1).astype(f)[:, None]
  cx, cy = f(W / 2), f(H / 2)
  dx = (qx + f(0.5)) * f(0.5) - cx
  dy = (qy + f(0.5)) * f(0.5) - cy
  a00, a01, a10, a11 = (f(v) for v in p[2:6])
  ux = ((a00 * dx + a01 * dy) + cx) + f(t0)
  uy = ((a10 * dx + a11 * dy) + cy) + f(t1)
  sx = f(2) * ux - f(0.5)
  sy = f(2) * uy - f(0.5)
  red0, red1 = float(reduced_translation(p[6], W)), float(reduced_translation(p[7], H))
  d64x, d64y = dx.astype(np.float64), dy.astype(np.float64)
  Mx = abs(float(p[2])) * np.abs(d64x) + abs(float(p[3])) * np.abs(d64y) + W / 2 + abs(red0)
  My = abs(float(p[4])) * np.abs(d64x) + abs(float(p[5])) * np.abs(d64y) + H / 2 + abs(red1)
  return sx, sy, Mx, My


def _up_axis(B, f, axis, dtype):
  """U along `axis` of an array B padded by m pixels there: index j' of the result is U[j' - 2 m]."""
  B = np.moveaxis(B, axis, -1)
  n = B.shape[-1]
  T, h = len(f), len(f) // 2
  Z = np.zeros(B.shape[:-1] + (2 * n,), dtype=dtype)
  Z[..., ::2] = B
  full = np.zeros(B.shape[:-1] + (2 * n + T - 1,), dtype=dtype)      # the full convolution, full[t] = sum_k f[k] Z[t - k]
  started = np.zeros(full.shape, dtype=bool)
  for k in range(T):
    term = dtype(f[k]) * Z
    seg = full[..., k:k + 2 * n]
    nz = np.zeros(seg.shape, dtype=bool)
    nz[..., ::2] = True                                              # the taps that meet a zero of Z are left out
    st = started[..., k:k + 2 * n]
    seg[...] = np.where(nz, np.where(st, seg + term, term), seg)
    st |= nz
  U = dtype(2) * full[..., h - 1:h - 1 + 2 * n]
  return np.moveaxis(U, -1, axis)


def _down_axis(V, f, axis, n, dtype):
  """O[i] = sum_k f[k] V[2i + k] along `axis` (V on its storage grid, index 0 = lattice index -(h - 1))."""
  V = np.moveaxis(V, axis, -1)
  acc = None
  for k in range(len(f)):
    term = dtype(f[k]) * V[..., k:k + 2 * n:2]
    acc = term if acc is None else acc + term
  return np.moveaxis(acc, -1, axis)


def warp(S, p, f, dtype=np.float64, reduce=False, parts=False):
  """The operator on one plane S [H, W] with the fp32 row p [8] and the fp32 taps f.  parts: also return (U, margin, V)."""
  H, W = S.shape
  T, h = len(f), len(f) // 2
  B = S[::-1] if p[1] != 0 else S
  B = B[:, ::-1] if p[0] != 0 else B
  B = np.ascontiguousarray(B).astype(dtype)
  if is_identity(p) and not parts:
    return B.copy()
  sx, sy, _, _ = _coords(p, H, W, T, dtype, reduce)
  # the margin, from this case's own matrix: the bilinear gather reads U[floor(s)] and U[floor(s) + 1], U[j] reads the
  # pixels (j - h) / 2 .. (j + h - 1) / 2, and the full convolution is complete h samples inside the padded array
  lo = min(float(sx.min()), float(sy.min()))
  hi = max(float(sx.max()) - 2 * W, float(sy.max()) - 2 * H)
  m = int(np.ceil(max(0.0, -lo, hi) / 2.0)) + h + 2
  Bp = np.pad(B, m, mode='reflect')
  U = _up_axis(Bp, f, 1, dtype)
  U = _up_axis(U, f, 0, dtype)
  bx, by = np.floor(sx), np.floor(sy)
  gx, gy = sx - bx, sy - by
  x0 = np.broadcast_to(bx.astype(np.int64) + 2 * m, (sy.shape[0], sx.shape[1]))
  y0 = np.broadcast_to(by.astype(np.int64) + 2 * m, x0.shape)
  gx, gy = np.broadcast_to(gx, x0.shape), np.broadcast_to(gy, x0.shape)
  one = dtype(1)
  hx, hy = one - gx, one - gy
  V = ((hy * hx) * U[y0, x0] + (hy * gx) * U[y0, x0 + 1]) + ((gy * hx) * U[y0 + 1, x0] + (gy * gx) * U[y0 + 1, x0 + 1])
  O = _down_axis(_down_axis(V, f, 1, W, dtype), f, 0, H, dtype)
  if parts:
    return O, U, m, V
  return O


def bound(S, p, f):
  """The allowed |kernel - warp(S, p, f)| per element, [H, W] float64 (the module docstring derives it)."""
  H, W = S.shape
  T = len(f)
  if is_identity(p):
    return np.zeros((H, W))
  af = np.abs(np.asarray(f, dtype=np.float32))
  P = warp(np.abs(S), p, af)
  n = 3 * T + 5
  gamma = n * EPS / (1 - n * EPS)
  _, U, m, _ = warp(S, p, f, parts=True)
  tile = U[2 * m - 1:2 * m + 2 * H + 1, 2 * m - 1:2 * m + 2 * W + 1]       # U[-1 .. 2n] per axis: every step of the lattice
  L = max(np.abs(np.diff(tile, axis=0)).max(), np.abs(np.diff(tile, axis=1)).max())
  _, _, Mx, My = _coords(p, H, W, T, np.float64, False)
  delta = EPS * (10 * (Mx + My) + 2) / (1 - 8 * EPS)
  E = _down_axis(_down_axis(L * delta, af, 1, W, np.float64), af, 0, H, np.float64)
  return gamma * P + E


def apply(x, params, f, dtype=np.float64, reduce=False):
  """warp over a batch: x [B, C, H, W], params [B, 8]."""
  x = np.asarray(x)
  return np.stack([np.stack([warp(x[b, c], params[b], f, dtype, reduce) for c in range(x.shape[1])]) for b in range(x.shape[0])])


def bounds(x, params, f):
  x = np.asarray(x)
  return np.stack([np.stack([bound(x[b, c], params[b], f) for c in range(x.shape[1])]) for b in range(x.shape[0])])


def image(B, C, H, W, seed=0):
  """Test planes that look like images: a few low harmonics per plane plus 2 % of white noise, fp32.  (The coordinate term of
  the bound is proportional to the steepest step of U; white noise alone would make the bound say little.)"""
  g = np.random.default_rng(seed)
  y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing='ij')
  out = np.zeros((B, C, H, W))
  for b in range(B):
    for c in range(C):
      for _ in range(3):
        ky, kx = g.integers(0, 3, 2)
        out[b, c] += g.normal() * np.cos(2 * np.pi * (ky * y + kx * x) + g.uniform(0, 2 * np.pi))
      out[b, c] += 0.02 * g.normal(size=(H, W))
  return out.astype(np.float32)


def rows(H, W):
  """name -> fp32 parameter row: each isolates one thing; the scaled, rotated and translated ones carry the sampling point
  across several reflection periods."""
  aniso = rot(30) @ np.diag([2.0 ** 1.2, 2.0 ** -1.2]) @ rot(-30)
  combined = aniso @ rot(73) @ (1.3 * np.eye(2))
  return {
    'identity': row(),
    'xflip': row(fx=1),
    'yflip': row(fy=1),
    'scale0.5': row(G=0.5 * np.eye(2)),
    'scale2.5': row(G=2.5 * np.eye(2)),
    'rot90': row(G=rot(90)),
    'rot45': row(G=rot(45)),
    'rot179': row(G=rot(179)),
    'aniso': row(G=aniso),
    'shift+3': row(shift=(3.0 * W + 0.3, 0.0)),
    'shift-3': row(shift=(0.0, -3.0 * H - 0.7)),
    'combined': row(fx=1, fy=1, G=combined, shift=(0.37 * W, -0.21 * H)),
  }
