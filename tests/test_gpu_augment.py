"""The entries of include/stk_augment.h on the device.

The warp: every element against the literal float64 restatement of tests/_augment_ref.py (reflect padding by a margin, zero
stuffing, full convolution, gather, decimation: none of the kernel's periodic indexing), within the bound derived there --
gamma_n P(|S|; |f|) + D(L (delta_x + delta_y); |f|), which stays below 1e-4 max|S| while an indexing error is 0.1 max|S|.
Rows that each isolate one thing, on every shape and tap count; identity rows bit for bit; two launches, the same bits; guard
bands; every error code before any launch.  The embedding pair: against float64 and bit for bit against its stated order."""
import ctypes

import numpy as np
import pytest
import torch

import _augment_ref as R
from _util import call

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 8), (5, 3, 8, 12), (3, 3, 32, 32), (2, 1, 64, 64)]
FILTERS = {'box2': R.box_filter(2), 'tent4': R.tent4(), 'kaiser12': R.default_filter()}
STK_EINVAL, STK_EUNSUPPORTED = -1, -3
GUARD = 64
_cache = {}


def _taps(f):
  return (ctypes.c_float * len(f))(*[float(v) for v in f])


def _launch(lib, x, params, f, guard=GUARD):
  """y of one launch, with `guard` sentinel floats on either side of it: (y, the whole buffer)."""
  B, C, H, W = x.shape
  buf = torch.full((x.numel() + 2 * guard,), -777.0, device=x.device)
  y = buf[guard:guard + x.numel()].view(B, C, H, W)
  taps = _taps(f)
  rc = lib.aug_warp_f32.raw(x.data_ptr(), params.data_ptr(), ctypes.cast(taps, ctypes.c_void_p), len(f), y.data_ptr(), B, C, H, W,
                            torch.cuda.current_stream().cuda_stream)
  assert rc == 0, rc
  return y, buf


def _case(shape, fname):
  """The launches of one (shape, filter): the 12 rows of _augment_ref.rows in batches of B (the last one wraps round), with
  the float64 reference and the bound of each, computed once."""
  key = (shape, fname)
  if key not in _cache:
    B, C, H, W = shape
    f = FILTERS[fname]
    rows = R.rows(H, W)
    names = list(rows)
    launches = []
    for l in range(-(-len(names) // B)):
      chosen = [names[(l * B + b) % len(names)] for b in range(B)]
      x = R.image(B, C, H, W, seed=1000 * l + H + W)
      params = np.stack([rows[n] for n in chosen])
      launches.append((chosen, x, params, R.apply(x, params, f), R.bounds(x, params, f)))
    _cache[key] = launches
  return _cache[key]


@pytest.mark.parametrize('fname', list(FILTERS))
@pytest.mark.parametrize('shape', SHAPES)
def test_warp_against_float64_per_element(hip_lib, shape, fname):
  dev = torch.device('cuda:0')
  f = FILTERS[fname]
  seen = set()
  for chosen, x, params, ref, bd in _case(shape, fname):
    xd, pd = torch.from_numpy(x).to(dev), torch.from_numpy(params).to(dev)
    y, buf = _launch(hip_lib, xd, pd, f)
    y2, _ = _launch(hip_lib, xd, pd, f)
    torch.cuda.synchronize()
    got = y.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert torch.equal(y, y2), 'two launches on the same operands differ'
    assert bool((buf[:GUARD] == -777.0).all()) and bool((buf[-GUARD:] == -777.0).all()), 'a guard band was written'
    for b, name in enumerate(chosen):
      seen.add(name)
      if R.is_identity(params[b]):
        assert np.array_equal(got[b], ref[b]), f'{name}: the exact path is not the flipped input bit for bit'
        continue
      rel = max(bd[b, c].max() / np.abs(x[b, c]).max() for c in range(x.shape[1]))
      assert rel < 1e-4, (name, rel)
      err = np.abs(got[b] - ref[b])
      ratio = float((err / bd[b]).max())
      print(f'{shape} {fname} {name}: max err {err.max():.3e}, worst err/bound {ratio:.3f}, bound/max|S| {rel:.2e}')
      assert ratio <= 1.0, f'{name}: error {err.max():.3e} is {ratio:.2f} of the bound'
  assert seen == set(R.rows(8, 8)), 'a row of the list was not run'


def test_the_pipe_runs_the_same_kernel(st, hip_lib):
  """AugmentPipe on the device: its output is the reference applied with ITS draws (replayed from a pipe of the same seed),
  the labels arrive, a p = 0 pipe returns the images bit for bit, and the device generator is not consumed."""
  dev = torch.device('cuda:0')
  B, C, H, W = 6, 3, 32, 32
  x = R.image(B, C, H, W, seed=42)
  xd = torch.from_numpy(x).to(dev)
  torch.cuda.manual_seed(5)
  before = torch.cuda.get_rng_state()
  pipe, twin = st.augment.AugmentPipe(0.7, seed=9), st.augment.AugmentPipe(0.7, seed=9)
  y, labels = pipe(xd)
  params, want_labels = twin.draw(B, H, W)
  assert torch.equal(torch.cuda.get_rng_state(), before)
  assert labels.shape == (B, 9) and torch.equal(labels.cpu(), want_labels)
  f = pipe.filter
  ref, bd = R.apply(x, params.numpy(), f), R.bounds(x, params.numpy(), f)
  got = y.cpu().numpy().astype(np.float64)
  moved = [b for b in range(B) if not R.is_identity(params[b].numpy())]
  assert moved, 'no sample of this draw has a geometric part'
  for b in range(B):
    if b in moved:
      assert (np.abs(got[b] - ref[b]) <= bd[b]).all(), b
    else:
      assert np.array_equal(got[b], ref[b]), b
  y0, l0 = st.augment.AugmentPipe(0.0)(xd)
  assert torch.equal(y0, xd) and not l0.any()


def test_error_codes_come_back_before_any_launch(hip_lib):
  dev = torch.device('cuda:0')
  warp = hip_lib.aug_warp_f32.raw
  stream = torch.cuda.current_stream().cuda_stream
  x = torch.zeros(2 * 3 * 66 * 66, device=dev)
  y = torch.full_like(x, -777.0)
  p = torch.from_numpy(np.stack([R.rows(8, 8)['rot45']] * 2)).to(dev)
  f12, f14, f2 = _taps(R.default_filter()), _taps(np.full(14, 1 / 14)), _taps([0.5, 0.5])
  bad = _taps([0.1, 0.2, 0.3, 0.4])
  nan = _taps([float('nan'), float('nan')])
  X, Y, Pp = x.data_ptr(), y.data_ptr(), p.data_ptr()
  vp = lambda t: ctypes.cast(t, ctypes.c_void_p)
  assert warp(X, Pp, vp(f12), 12, Y, 2, 3, 32, 32, stream) == 0
  torch.cuda.synchronize()
  y.fill_(-777.0)
  for args, want in (
      ((None, Pp, vp(f12), 12, Y, 2, 3, 32, 32), STK_EINVAL), ((X, None, vp(f12), 12, Y, 2, 3, 32, 32), STK_EINVAL),
      ((X, Pp, None, 12, Y, 2, 3, 32, 32), STK_EINVAL), ((X, Pp, vp(f12), 12, None, 2, 3, 32, 32), STK_EINVAL),
      ((X, Pp, vp(f12), 12, Y, 0, 3, 32, 32), STK_EINVAL), ((X, Pp, vp(f12), 12, Y, 2, 0, 32, 32), STK_EINVAL),
      ((X, Pp, vp(f12), 12, Y, 2, 3, 0, 32), STK_EINVAL), ((X, Pp, vp(f12), 0, Y, 2, 3, 32, 32), STK_EINVAL),
      ((X, Pp, vp(nan), 2, Y, 2, 3, 32, 32), STK_EINVAL),
      ((X, Pp, vp(f12), 12, Y, 2, 3, 66, 64), STK_EUNSUPPORTED), ((X, Pp, vp(f12), 12, Y, 2, 3, 64, 66), STK_EUNSUPPORTED),
      ((X, Pp, vp(f12), 12, Y, 2, 3, 32, 31), STK_EUNSUPPORTED), ((X, Pp, vp(f12), 12, Y, 2, 3, 31, 32), STK_EUNSUPPORTED),
      ((X, Pp, vp(f12), 12, Y, 2, 3, 6, 8), STK_EUNSUPPORTED), ((X, Pp, vp(f14), 14, Y, 2, 3, 32, 32), STK_EUNSUPPORTED),
      ((X, Pp, vp(f12), 3, Y, 2, 3, 32, 32), STK_EUNSUPPORTED), ((X, Pp, vp(bad), 4, Y, 2, 3, 32, 32), STK_EUNSUPPORTED),
      ((X, Pp, vp(f2), 2, Y, 1 << 16, 1 << 15, 8, 8), STK_EUNSUPPORTED)):
    assert warp(*args, stream) == want, args[3:]
  torch.cuda.synchronize()
  assert bool((y == -777.0).all()), 'a refused call launched something'
  for H, W, T, ok in ((8, 8, 2, 1), (64, 64, 12, 1), (8, 12, 4, 1), (66, 64, 12, 0), (32, 31, 12, 0), (32, 32, 14, 0), (32, 32, 3, 0)):
    assert hip_lib.aug_ok(H, W, T) == ok
  # the embedding pair
  fwd, bwd = hip_lib.aug_embed_fwd_f32.raw, hip_lib.aug_embed_bwd_f32.raw
  t = torch.zeros(4 * 8, device=dev)
  T_ = t.data_ptr()
  assert fwd(None, T_, T_, T_, 2, 2, 2, stream) == STK_EINVAL and fwd(T_, T_, T_, None, 2, 2, 2, stream) == STK_EINVAL
  assert fwd(T_, T_, T_, T_, 0, 2, 2, stream) == STK_EINVAL and fwd(T_, T_, T_, T_, 2, 2, 0, stream) == STK_EINVAL
  assert fwd(T_, T_, T_, T_, 1 << 16, 2, 1 << 15, stream) == STK_EUNSUPPORTED
  assert bwd(T_, T_, None, 0.0, None, 2, 2, 2, stream) == STK_EINVAL and bwd(None, T_, T_, 0.0, T_, 2, 2, 2, stream) == STK_EINVAL
  assert bwd(T_, T_, T_, 0.5, T_, 2, 2, 2, stream) == STK_EINVAL and bwd(T_, T_, T_, 0.0, T_, 2, 0, 2, stream) == STK_EINVAL
  assert bwd(T_, T_, T_, 1.0, T_, 1 << 16, 2, 1 << 15, stream) == STK_EUNSUPPORTED
  torch.cuda.synchronize()
  assert not t.any()


EMBED_SHAPES = [(1, 9, 4), (5, 9, 130), (128, 9, 512)]


def _embed_operands(B, K, D):
  g = torch.Generator().manual_seed(B + D)
  t = torch.randn(B, D, generator=g)
  labels = torch.randn(B, K, generator=g)
  labels[torch.rand(B, K, generator=g) < 0.5] = 0.0          # most labels of a real batch are zeros
  Wt = torch.randn(D, K, generator=g) * 0.3
  gy = torch.randn(B, D, generator=g)
  gt0 = torch.randn(B, D, generator=g)
  gW0 = torch.randn(D, K, generator=g)
  return t, labels, Wt, gy, gt0, gW0


@pytest.mark.parametrize('shape', EMBED_SHAPES)
def test_embed_forward(hip_lib, shape):
  B, K, D = shape
  dev = torch.device('cuda:0')
  t, labels, Wt, *_ = _embed_operands(B, K, D)
  y = torch.full((B * D + 2 * GUARD,), -777.0, device=dev)
  out = y[GUARD:GUARD + B * D].view(B, D)
  call(hip_lib, 'aug_embed_fwd_f32', t.to(dev), labels.to(dev), Wt.to(dev), out, B, K, D)
  got = out.cpu()
  assert bool((y[:GUARD] == -777.0).all()) and bool((y[-GUARD:] == -777.0).all())
  # the stated order in numpy fp32: acc = l0 w0; acc += lk wk, k ascending; y = t + acc -- bit for bit
  l, w = labels.numpy(), Wt.numpy()
  acc = l[:, None, 0] * w[None, :, 0]
  for k in range(1, K):
    acc = acc + l[:, None, k] * w[None, :, k]
  want32 = t.numpy() + acc
  assert acc.dtype == np.float32 and np.array_equal(got.numpy(), want32)
  # float64: K products and K sums meet the first term at most
  ref = t.double() + labels.double() @ Wt.double().T
  mag = t.double().abs() + labels.double().abs() @ Wt.double().abs().T
  assert bool(((got.double() - ref).abs() <= (K + 1) * 2.0 ** -24 * mag).all())
  # in place
  td = t.to(dev)
  call(hip_lib, 'aug_embed_fwd_f32', td, labels.to(dev), Wt.to(dev), td, B, K, D)
  assert torch.equal(td.cpu(), got)


@pytest.mark.parametrize('beta', [0.0, 1.0])
@pytest.mark.parametrize('shape', EMBED_SHAPES)
def test_embed_backward(hip_lib, shape, beta):
  B, K, D = shape
  dev = torch.device('cuda:0')
  t, labels, Wt, gy, gt0, gW0 = _embed_operands(B, K, D)
  want_gt = gy.numpy() if beta == 0 else gt0.numpy() + gy.numpy()
  # b ascending from the value already there, each product and sum rounded once
  acc = gW0.numpy().copy()
  l, g = labels.numpy(), gy.numpy()
  for b in range(B):
    acc = acc + g[b][:, None] * l[b][None, :]
  assert acc.dtype == np.float32
  ref = gW0.double() + gy.double().T @ labels.double()
  mag = gW0.double().abs() + gy.double().abs().T @ labels.double().abs()
  for want_t, want_w in ((True, True), (True, False), (False, True)):
    gt = gt0.clone().to(dev) if want_t else None
    if want_t and beta == 0:
      gt.fill_(float('nan'))                                    # beta = 0 does not read gt
    gW = gW0.clone().to(dev) if want_w else None
    call(hip_lib, 'aug_embed_bwd_f32', gy.to(dev), labels.to(dev), gt, beta, gW, B, K, D)
    if want_t:
      assert np.array_equal(gt.cpu().numpy(), want_gt)
    if want_w:
      assert np.array_equal(gW.cpu().numpy(), acc), 'the weight gradient is not the stated order bit for bit'
      assert bool(((gW.cpu().double() - ref).abs() <= (B + 1) * 2.0 ** -24 * mag).all())
