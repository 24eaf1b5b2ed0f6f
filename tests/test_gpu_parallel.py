"""The three launches of include/stk_parallel.h (csrc/parallel.hip) and the parallel-in-time sampler built on them
(soft-truncation_amd/parallel_sampling.py), on the device.

The scan, the slide and the loop with a linear score are held to the numpy fp32 restatement of tests/_parallel_ref.py BIT FOR
BIT: every product and sum is rounded once, in the order the header writes them, and the sums along the slots are strictly
sequential, so there is nothing to tolerate.  The error sums are float64 sums of n non-negative fp32 squares in some fixed
order: any order is within (n - 1) 2^-53 relative of the exact sum, which math.fsum gives.  The stride decisions of the loop
are the restatement's because test_parallel_cpu.py holds every decision of that case at least 1e-3 relative from its
threshold, six orders of magnitude above what the order of a float64 sum can move.

The sampler on the tiny networks, against float64 loops: the tolerance is measured, not fixed in advance -- the float64
by-hand loop (same engine score function, same batch, the recorded strides replayed) is run again in torch fp32, and four times
its deviation from float64 is what the sampler may deviate (the rule of test_gpu_dpm_solver.py).  It is held at tol = 0 and
tol = 1e30 (every slot accepted): neither has a decision near a threshold.  The deviations are printed by the tests.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

import _parallel_ref as R
from _model_util import randomize_, tiny_config
from _sampler_util import sampler, setup, shape_of
from _stream_util import Guarded, ptr, stream

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
EPS = 1e-3
DEV = torch.device('cuda:0')
f32 = lambda v: np.asarray(v, dtype=np.float32)


def _ws_parts(lib, W, B, n):
  nbytes = int(lib.picard_ws_bytes(W, B, n))
  assert nbytes > 0 and nbytes % (8 * B * W) == 0
  return nbytes, nbytes // (8 * B * W)


def _operands(W, B, n, rows, seed):
  rng = np.random.RandomState(seed)
  X = f32(rng.standard_normal((W + 1, B, n)) * 1.5)
  S = f32(rng.standard_normal((W, B, n)) * 2.0)
  Z = f32(rng.standard_normal((W, B, n)))
  coef = f32(np.stack([-0.1 + 0.05 * rng.standard_normal(rows), 0.2 + 0.1 * rng.standard_normal(rows),
                       0.4 + 0.1 * rng.standard_normal(rows)], axis=1))
  return X, S, Z, coef


def _scan_case(lib, W, p, B, n, i0, noise, placement, seed):
  """One launch against the restatement; returns the number of elements compared."""
  what = f'scan W={W} p={p} B={B} n={n} i0={i0} noise={noise} {placement}'
  X, S, Z, coef = _operands(W, B, n, i0 + p, seed)                     # the table ends where the window does
  nbytes, parts = _ws_parts(lib, W, B, n)
  gX, gS, gZ = (Guarded(t, DEV, placement) for t in (X, S, Z))
  gws = Guarded(torch.full((B, W, parts), float('nan'), dtype=torch.float64), DEV)
  gerr = Guarded(torch.full((W,), float('nan'), dtype=torch.float64), DEV)
  coef_d = torch.from_numpy(coef).to(DEV)
  lib.picard_scan_f32(gX.view.data_ptr(), gS.view.data_ptr(), gZ.view.data_ptr() if noise else None, coef_d.data_ptr(), i0, p, W,
                      gws.view.data_ptr(), nbytes, B, n, stream())
  thr = torch.zeros(i0 + p, dtype=torch.float64, device=DEV)
  stride = torch.full((1,), -7, dtype=torch.int32, device=DEV)
  lib.picard_stride(gws.view.data_ptr(), nbytes, thr.data_ptr(), i0, p, W, B, n, stride.data_ptr(), gerr.view.data_ptr(), stream())
  torch.cuda.synchronize()
  for g in (gX, gS, gZ, gws, gerr):
    g.check(what)
  Y, _ = R.scan(X, S, Z if noise else None, coef, i0, p, W)
  want = X.copy()
  want[1:p + 1] = Y[1:]                                                # X[0] and the slots beyond p stay
  got = gX.view.cpu().numpy()
  assert got.tobytes() == want.tobytes(), f'{what}: {int((got != want).sum())} elements differ from the fp32 restatement'
  assert torch.equal(gS.view.cpu(), torch.from_numpy(S)) and torch.equal(gZ.view.cpu(), torch.from_numpy(Z)), what
  ws = gws.view.cpu().numpy()
  assert np.isfinite(ws).all(), f'{what}: a workspace entry was not written'
  err = np.zeros((B, W))
  for k in range(parts):                                               # the stride kernel's order: index order
    err = err + ws[:, :, k]
  assert not err[:, 0].any() and not err[:, p:].any(), f'{what}: slot 0 and the padding carry no error'
  for j in range(1, p):
    r = Y[j] - X[j]
    squares = (r * r).astype(np.float64)
    assert r.dtype == np.float32 and (r * r).dtype == np.float32
    for b in range(B):
      exact = math.fsum(squares[b])
      assert abs(err[b, j] - exact) <= (n - 1) * 2. ** -53 * exact, (what, b, j, err[b, j], exact)
  assert np.array_equal(gerr.view.cpu().numpy(), err.max(axis=0)), f'{what}: err_out is not the largest error over b'
  assert int(stride) == 1 + next((k for k in range(p - 1) if err[:, k + 1].max() > 0), p - 1), what
  return B * n * p


@pytest.mark.parametrize('n', [1, 5, 64, 4 * 300, 4 * 300 + 2])
def test_scan_matches_the_fp32_restatement(hip_lib, n):
  """W in {1, 2, 8, 9, 17} around the group of 8 slots, p = W and p < W, B in {1, 3}; 16-byte path (n % 4 == 0, aligned),
  scalar path (odd n, or a pointer entered 4 bytes), more than one block per row (n = 1200: 2 vector, 5 scalar blocks)."""
  seen = 0
  for W in (1, 2, 8, 9, 17):
    for p in sorted({W, max(1, W - 1)}):
      for B in (1, 3):
        seen += _scan_case(hip_lib, W, p, B, n, 0, True, 'aligned', seed=W * 100 + p * 10 + B)
  for placement in ('entered-one-in', 'aligned'):
    seen += _scan_case(hip_lib, 8, 7, 3, n, 5, True, placement, seed=1)   # i0 > 0: the ring wraps at slot 3
    seen += _scan_case(hip_lib, 17, 17, 1, n, 30, True, placement, seed=2)
    seen += _scan_case(hip_lib, 9, 9, 3, n, 4, False, placement, seed=3)  # Z = NULL
    seen += _scan_case(hip_lib, 1, 1, 1, n, 0, False, placement, seed=4)
  print(f'n = {n}: {seen} element-slots bit for bit')


@pytest.mark.parametrize('placement', ['aligned', 'entered-one-in'])
def test_scan_and_slide_when_a_block_walks_its_row_more_than_once(hip_lib, placement):
  """B = 16 rows of n = 3 x 256 x 256 + 8: 128 blocks share a row of 49154 float4 items (two passes, the second with two live
  threads in its last block) or, entered 4 bytes, of 196616 scalar items (seven passes, eight live threads at the end): the
  per-slot sums accumulate across passes, and threads past the row's end contribute and store nothing.  The slide's grid of
  2048 blocks strides its 786464 / 3145856 items too."""
  W, B, n = 3, 16, 3 * 256 * 256 + 8
  nbytes, parts = _ws_parts(hip_lib, W, B, n)
  assert parts == 128 and parts * 256 < n // 4
  for p, i0, noise in ((3, 2, True), (2, 0, False)):
    _scan_case(hip_lib, W, p, B, n, i0, noise, placement, seed=p)
  X = f32(np.random.RandomState(5).standard_normal((W + 1, B, n)))
  for p, given in ((3, 1), (3, 2), (2, 2)):
    g = Guarded(X, DEV, placement)
    stride = torch.full((1,), given, dtype=torch.int32, device=DEV)
    hip_lib.picard_slide_f32(g.view.data_ptr(), stride.data_ptr(), p, W, B, n, stream())
    torch.cuda.synchronize()
    g.check(f'slide p={p} s={given}')
    want = np.stack([X[min(j + given, p)] for j in range(W + 1)])
    assert g.view.cpu().numpy().tobytes() == want.tobytes(), (p, given)


def test_scan_that_has_converged_reports_zero_error(hip_lib):
  """X already the prefix sums: Y = X bit for bit, every error exactly 0, the stride is p."""
  W, B, n = 9, 2, 68
  X, S, Z, coef = _operands(W, B, n, W, 11)
  Y, _ = R.scan(X, S, Z, coef, 0, W, W)
  for _ in range(W):                                                   # iterate to the fixed point of these fixed scores
    X = Y.copy()
    Y, err = R.scan(X, S, Z, coef, 0, W, W)
  assert not err.any()
  nbytes, parts = _ws_parts(hip_lib, W, B, n)
  Xd, Sd, Zd, cd = (torch.from_numpy(v).to(DEV) for v in (X, S, Z, coef))
  ws = torch.full((B, W, parts), float('nan'), dtype=torch.float64, device=DEV)
  hip_lib.picard_scan_f32(Xd.data_ptr(), Sd.data_ptr(), Zd.data_ptr(), cd.data_ptr(), 0, W, W, ws.data_ptr(), nbytes, B, n, stream())
  assert np.array_equal(Xd.cpu().numpy(), X) and not bool(ws.any())
  stride = torch.zeros(1, dtype=torch.int32, device=DEV)
  thr = torch.zeros(W, dtype=torch.float64, device=DEV)
  hip_lib.picard_stride(ws.data_ptr(), nbytes, thr.data_ptr(), 0, W, W, B, n, stride.data_ptr(), None, stream())
  assert int(stride) == W


# ---- the stride on crafted workspaces ------------------------------------------------------------------------------------
def _stride(lib, err, thr, i0, p, W, B, n, seed=0, want_err=True):
  """err [B, W] float64 spread over the workspace (one random block carries each value, so the sums are exact)."""
  nbytes, parts = _ws_parts(lib, W, B, n)
  rng = np.random.RandomState(seed)
  ws = np.zeros((B, W, parts))
  for b in range(B):
    for j in range(W):
      ws[b, j, rng.randint(parts)] = err[b, j]
  gws = Guarded(ws, DEV)
  out = torch.full((3,), -7, dtype=torch.int32, device=DEV)         # the stride goes to the middle one
  gerr = Guarded(torch.full((W,), float('nan'), dtype=torch.float64), DEV)
  thr_d = torch.from_numpy(np.asarray(thr, dtype=np.float64)).to(DEV)
  lib.picard_stride(gws.view.data_ptr(), nbytes, thr_d.data_ptr(), i0, p, W, B, n, out[1:].data_ptr(),
                    gerr.view.data_ptr() if want_err else None, stream())
  torch.cuda.synchronize()
  gws.check('stride')
  gerr.check('stride')
  assert out[0] == -7 and out[2] == -7
  assert gws.view.cpu().numpy().tobytes() == ws.tobytes(), 'the workspace was written'
  return int(out[1]), gerr.view.cpu().numpy()


@pytest.mark.parametrize('W,p,B,n', [(8, 8, 1, 64), (9, 7, 3, 1200), (17, 17, 2, 5), (1, 1, 2, 64), (256, 256, 1, 8)])
def test_stride_counts_the_leading_converged_slots(hip_lib, W, p, B, n):
  i0 = 3
  rng = np.random.RandomState(W + p)
  thr = np.concatenate([np.full(i0, np.nan), np.exp(rng.uniform(-3, 3, size=W))])    # entries below i0 are not the window's
  below = lambda: thr[None, i0:] * rng.uniform(0., 0.999, size=(B, W))
  for want in range(1, p + 1):
    err = below()
    err[:, p:] = np.nan                                                # the padding is ignored, whatever it holds
    err[:, 0] = np.inf                                                 # ... and so is slot 0
    if want < p:
      err[rng.randint(B), want] = thr[i0 + want] * 1.5                 # one sample of B fails alone; later slots pass again
    got, worst = _stride(hip_lib, err, thr, i0, p, W, B, n, seed=want)
    assert got == want, (W, p, B, want, got)
    assert np.array_equal(worst[1:p], err[:, 1:p].max(axis=0)) and worst[0] == 0. and not worst[p:].any()
  if p >= 3:
    base = below()
    at = base.copy()
    at[B - 1, 2] = thr[i0 + 2]                                         # exactly at the threshold: converged
    assert _stride(hip_lib, at, thr, i0, p, W, B, n)[0] == p
    above = base.copy()
    above[B - 1, 2] = np.nextafter(thr[i0 + 2], np.inf)                # one ulp above: not
    assert _stride(hip_lib, above, thr, i0, p, W, B, n)[0] == 2
    bad = base.copy()
    bad[0, 1] = np.nan                                                 # a NaN is not converged
    got, worst = _stride(hip_lib, bad, thr, i0, p, W, B, n)
    assert got == 1 and np.isnan(worst[1]) and np.array_equal(worst[2:p], bad[:, 2:p].max(axis=0))
    zero = np.zeros((B, W))
    assert _stride(hip_lib, zero, np.zeros(i0 + W), i0, p, W, B, n, want_err=False)[0] == p      # 0 <= 0: tol = 0 accepts exact slots
    tiny = zero.copy()
    tiny[0, 1] = 5e-324
    assert _stride(hip_lib, tiny, np.zeros(i0 + W), i0, p, W, B, n)[0] == 1
    assert _stride(hip_lib, np.full((B, W), np.inf), np.full(i0 + W, np.inf), i0, p, W, B, n)[0] == p


# ---- the slide ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [5, 64, 4 * 300])
@pytest.mark.parametrize('placement', ['aligned', 'entered-one-in'])
def test_slide_for_every_stride(hip_lib, n, placement):
  for W, B in ((1, 2), (8, 1), (9, 3), (17, 2)):
    for p in sorted({W, max(1, W - 1)}):
      X = f32(np.random.RandomState(W + p).standard_normal((W + 1, B, n)))
      for given in list(range(1, p + 1)) + [0, -5, p + 3]:
        s = min(max(given, 1), p)                                      # the device value is clamped to [1, p]
        g = Guarded(X, DEV, placement)
        stride = torch.full((1,), given, dtype=torch.int32, device=DEV)
        hip_lib.picard_slide_f32(g.view.data_ptr(), stride.data_ptr(), p, W, B, n, stream())
        torch.cuda.synchronize()
        g.check(f'slide W={W} p={p} s={given}')
        want = np.stack([X[min(j + s, p)] for j in range(W + 1)])
        assert g.view.cpu().numpy().tobytes() == want.tobytes(), (W, p, B, n, given)
        assert int(stride) == given


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_return_codes_and_nothing_written(hip_lib):
  W, B, n, p, i0 = 8, 2, 64, 6, 2
  nbytes, parts = _ws_parts(hip_lib, W, B, n)
  X = torch.full((W + 1, B, n), 7.0, device=DEV)
  S, Z = torch.ones(W, B, n, device=DEV), torch.ones(W, B, n, device=DEV)
  coef = torch.ones(i0 + p, 3, device=DEV)
  ws = torch.full((B, W, parts), 7.0, dtype=torch.float64, device=DEV)
  thr = torch.ones(i0 + p, dtype=torch.float64, device=DEV)
  stride_out = torch.full((1,), 7, dtype=torch.int32, device=DEV)
  err_out = torch.full((W,), 7.0, dtype=torch.float64, device=DEV)
  sentinels = (X, ws, stride_out, err_out)

  def untouched():
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in sentinels), 'a refused call wrote'

  def scan(X=X, S=S, Z=Z, coef=coef, i0=i0, p=p, W=W, ws=ws, nbytes=nbytes, B=B, n=n, off=0):
    code = hip_lib.picard_scan_f32.raw(ptr(X), ptr(S), ptr(Z), ptr(coef), i0, p, W, None if ws is None else ws.data_ptr() + off,
                                       nbytes, B, n, stream())
    untouched()
    return code

  def decide(ws=ws, nbytes=nbytes, thr=thr, i0=i0, p=p, W=W, B=B, n=n, out=stride_out, err=err_out, off=0):
    code = hip_lib.picard_stride.raw(None if ws is None else ws.data_ptr() + off, nbytes, ptr(thr), i0, p, W, B, n, ptr(out),
                                     ptr(err), stream())
    untouched()
    return code

  def slide(X=X, s=stride_out, p=p, W=W, B=B, n=n):
    code = hip_lib.picard_slide_f32.raw(ptr(X), ptr(s), p, W, B, n, stream())
    untouched()
    return code

  for call in (scan, decide, slide):
    assert call(p=0) == EINVAL and call(p=W + 1) == EINVAL and call(p=-1) == EINVAL
    assert call(W=0, p=1) == EINVAL and call(B=0) == EINVAL and call(n=0) == EINVAL and call(n=-4) == EINVAL
    assert call(W=257, p=8) == EUNSUPPORTED
    assert call(n=2 ** 31) == EUNSUPPORTED and call(n=2 ** 28) == EUNSUPPORTED          # 9 x 2 x 2^28 >= 2^31
    assert call(W=256, p=8, B=2 ** 10, n=2 ** 13) == EUNSUPPORTED
  assert scan(X=None) == EINVAL and scan(S=None) == EINVAL and scan(coef=None) == EINVAL and scan(ws=None) == EINVAL
  assert scan(i0=-1) == EINVAL and scan(nbytes=nbytes - 8) == EINVAL and scan(nbytes=0) == EINVAL and scan(off=4) == EINVAL
  assert decide(ws=None) == EINVAL and decide(thr=None) == EINVAL and decide(out=None) == EINVAL
  assert decide(i0=-1) == EINVAL and decide(nbytes=nbytes - 8) == EINVAL and decide(off=4) == EINVAL
  assert slide(X=None) == EINVAL and slide(s=None) == EINVAL
  assert hip_lib.picard_ws_bytes(W, B, n) == nbytes
  # ... and the accepted edge forms run: no noise, no err_out, a larger workspace
  fresh = torch.ones(W + 1, B, n, device=DEV)
  big = torch.zeros(nbytes + 64, dtype=torch.uint8, device=DEV)
  assert hip_lib.picard_scan_f32.raw(fresh.data_ptr(), S.data_ptr(), None, coef.data_ptr(), i0, p, W, big.data_ptr(), nbytes + 64, B,
                                     n, stream()) == 0
  out = torch.zeros(1, dtype=torch.int32, device=DEV)
  assert hip_lib.picard_stride.raw(big.data_ptr(), nbytes + 64, thr.data_ptr(), i0, p, W, B, n, out.data_ptr(), None, stream()) == 0
  assert hip_lib.picard_slide_f32.raw(fresh.data_ptr(), out.data_ptr(), p, W, B, n, stream()) == 0
  torch.cuda.synchronize()
  assert 1 <= int(out) <= p
  with pytest.raises(RuntimeError, match='stk_picard_slide_f32 failed'):
    hip_lib.picard_slide_f32(None, out.data_ptr(), p, W, B, n, stream())


# ---- the loop with a linear score --------------------------------------------------------------------------------------------
SHAPE = (2, 3, 8, 8)                                                   # B = 2, n = 192: the case test_parallel_cpu.py checks


def _schedule(ps, case):
  """The restatement's own grid and float64 coefficients as the package's record: the loop rounds them exactly as
  the restatement does (picard_schedule agrees with them to 1e-9, test_parallel_cpu.py, which is not bit for bit)."""
  final = np.array([1. / case['alpha'][-1], case['sigma'][-1] ** 2 / case['alpha'][-1], 0., 0., 1.])
  return ps.PicardSchedule(sde_name=case['family'], steps=case['N'], eta=case['eta'], skip='time', times=case['times'],
                           alpha=case['alpha'], sigma=case['sigma'], coef=case['coef'], thr_unit=case['sigma'][:-1] ** 2, final=final)


def _linear_score(case, calls):
  """ONE fp32 multiply by the factor of the slot's time, looked up by exact equality with the grid's fp32 times."""
  times = torch.tensor(case['times'], dtype=torch.float32).to(DEV)
  factor = torch.tensor(case['factor'], dtype=torch.float32).to(DEV)

  def score_fn(x, t):
    assert t.shape == (x.shape[0],) and t.dtype == torch.float32 and t.device == x.device and x.is_contiguous()
    hit = t[:, None] == times[None, :]
    assert bool((hit.sum(dim=1) == 1).all()), 'a time that is not on the grid'
    calls.append(x.shape[0])
    return x * factor[hit.int().argmax(dim=1)][:, None, None, None]

  return score_fn


@pytest.mark.parametrize('family,eta', [(f, e) for f in ('vp', 've') for e in (0., 1.)])
def test_loop_is_the_restatement_bit_for_bit(st, hip_lib, monkeypatch, family, eta):
  ps = st.parallel_sampling
  case = R.gaussian_case(family, 100, eta, eps=EPS)
  x0, Z = R.draws(case, 2, 192)
  want = R.run(case, x0, Z, 16, 0.01, np.float32)
  served = []

  def randn(*size, dtype=None, device=None):
    assert tuple(size[0]) == SHAPE and dtype == torch.float32 and torch.device(device) == DEV
    served.append(len(served))
    return torch.from_numpy(f32(Z[len(served) - 1]).reshape(SHAPE)).to(DEV)

  monkeypatch.setattr(torch, 'randn', randn)
  calls = []
  x = torch.from_numpy(f32(x0).reshape(SHAPE)).to(DEV)
  out, stats = ps.parallel_sample(_linear_score(case, calls), x, _schedule(ps, case), 16, 0.01)
  assert out is x and served == (list(range(100)) if eta else []), 'the noise of step i is the (i + 1)-th draw'
  assert stats['strides'] == want['strides'] and stats['iterations'] == want['iterations'] == len(calls)
  assert stats['evaluations'] == want['evaluations'] and calls == [32] * len(calls)
  assert out.cpu().numpy().reshape(2, 192).tobytes() == want['x'].tobytes()
  print(f'{family} eta {eta}: {stats["iterations"]} iterations, {stats["evaluations"]} evaluations, strides {stats["strides"]}')


@pytest.mark.parametrize('family,eta', [(f, e) for f in ('vp', 've') for e in (0., 1.)])
def test_window_16_at_tolerance_zero_is_window_1(st, hip_lib, family, eta):
  """... under torch.manual_seed, with the generator left where the window = 1 run leaves it."""
  ps = st.parallel_sampling
  case = R.gaussian_case(family, 100, eta, eps=EPS)
  x0, _ = R.draws(case, 2, 192)
  outs = {}
  for W in (1, 16, 7):
    torch.manual_seed(5)
    x = torch.from_numpy(f32(x0).reshape(SHAPE)).to(DEV)
    out, stats = ps.parallel_sample(_linear_score(case, []), x, _schedule(ps, case), W, 0.)
    outs[W] = (out.cpu(), stats, torch.get_rng_state(), torch.cuda.get_rng_state())
  assert outs[1][1]['strides'] == [1] * 100 and outs[1][1]['evaluations'] == 100
  for W in (16, 7):
    assert torch.equal(outs[W][0], outs[1][0]), f'window {W} at tol = 0 is not the sequential run'
    assert torch.equal(outs[W][2], outs[1][2]) and torch.equal(outs[W][3], outs[1][3]), 'the generator ends elsewhere'
    assert outs[W][1]['iterations'] < 100 and sum(outs[W][1]['strides']) == 100
  torch.manual_seed(5)
  for _ in range(100 if eta else 0):
    torch.randn(SHAPE, dtype=torch.float32, device=DEV)
  assert torch.equal(torch.cuda.get_rng_state(), outs[16][3]), 'N draws for eta > 0, none for eta = 0'
  print(f'{family} eta {eta}: tol = 0 takes {outs[16][1]["iterations"]} iterations at window 16, {outs[7][1]["iterations"]} at 7')


# ---- the sampler on the tiny networks ---------------------------------------------------------------------------------------
STEPS, WINDOW = 12, 4


def _setup(st, lib, family):
  return setup(st, lib, family, dict(method='parallel', parallel_steps=STEPS, parallel_window=WINDOW, noise_removal=True))


def _family_marginal(st, sde):
  if isinstance(sde, st.sde_lib.VESDE):
    return lambda t: R.alpha_sigma('ve', t, sigma_min=sde.sigma_min, sigma_max=sde.sigma_max)
  return lambda t: R.alpha_sigma('vp', t, beta_min=sde.beta_0, beta_max=sde.beta_1)


@contextlib.contextmanager
def _window_conditions(model, W):
  """The test's own conditions of a window, built from the definition and not through models.utils.tiled_conditions: the
  classes in force W times over, slot-major, and under guidance [those; as many null classes]."""
  net = model.module
  saved = getattr(net, '_class_ctx', None)
  if saved is not None:
    cls, w, both = saved
    tiled = torch.cat([cls] * W)
    null = torch.full((W * cls.shape[0],), float(net.num_classes), dtype=torch.float32, device=cls.device)
    net._class_ctx = (tiled, w, None if both is None else torch.cat([tiled, null]))
  try:
    yield
  finally:
    if saved is not None:
      net._class_ctx = saved


def _by_hand(st, cfg, sde, model, eta, strides, dtype, seed, shape, context=()):
  """The test's own loop in torch `dtype`: the restatement's coefficients, the same engine score function at the same batch,
  the recorded strides replayed, the noise drawn as the sampler draws it."""
  mu = st.models.utils
  times = R.fp32(np.linspace(float(R.fp32(sde.T)), float(R.fp32(EPS)), STEPS + 1))
  alpha, sigma = _family_marginal(st, sde)(times)
  coef = R.coefficients(alpha, sigma, eta)
  if dtype == torch.float32:
    coef = f32(coef)
  score_fn = mu.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
  B, W, N = shape[0], WINDOW, STEPS
  torch.manual_seed(seed)
  with torch.no_grad():
    x = sde.prior_sampling(shape).to(cfg.device).to(dtype)
    X = [x] * (W + 1)
    ring = [None] * W
    i0 = entered = 0
    for stride in strides:
      p = min(W, N - i0)
      for i in range(entered, i0 + p if eta else entered):
        ring[i % W] = torch.randn(shape, dtype=torch.float32, device=cfg.device).to(dtype)
      entered = i0 + p
      t = torch.tensor([times[i0 + min(j, p - 1)] for j in range(W)], dtype=torch.float32, device=cfg.device).repeat_interleave(B)
      with _window_conditions(model, W):
        S = score_fn(torch.cat(X[:W]).float(), t).to(dtype)
      Y = [X[0]]
      for j in range(p):
        c0, c1, c2 = (float(v) for v in coef[i0 + j])
        d = c0 * X[j] + c1 * S[j * B:(j + 1) * B]
        if eta:
          d = d + c2 * ring[(i0 + j) % W]
        Y.append(Y[j] + d)
      X = [Y[min(j + stride, p)] for j in range(W + 1)]
      i0 += stride
    assert i0 == N
    x = X[0]
    cx, cs = 1. / alpha[-1], sigma[-1] ** 2 / alpha[-1]
    if dtype == torch.float32:
      cx, cs = float(np.float32(cx)), float(np.float32(cs))
    score = score_fn(x.float(), torch.full((B,), float(times[-1]), dtype=torch.float32, device=cfg.device)).to(dtype)
    return st.datasets.get_data_inverse_scaler(cfg)(cx * x + cs * score)


def _rel(a, b):
  a, b = a.detach().cpu().double(), b.detach().cpu().double()
  return float((a - b).abs().max() / b.abs().max())


def _evaluations(strides):
  total = i0 = 0
  for s in strides:
    total += min(WINDOW, STEPS - i0)
    i0 += s
  assert i0 == STEPS
  return total


@pytest.mark.parametrize('tol', [0., 1e30], ids=['tol0', 'accept-all'])
@pytest.mark.parametrize('eta', [0., 1.])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_sampler_matches_a_float64_loop(st, hip_lib, family, eta, tol):
  cfg, sde, model = _setup(st, hip_lib, family)
  shape = shape_of(cfg)
  fn = sampler(st, cfg, sde, EPS, parallel_tol=tol, parallel_eta=eta)
  assert fn.last_stats is None
  torch.manual_seed(3)
  got, nfe = fn(model)
  stats = fn.last_stats
  assert got.shape == shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
  assert stats['iterations'] == len(stats['strides']) <= STEPS and sum(stats['strides']) == STEPS
  assert nfe == stats['evaluations'] == _evaluations(stats['strides']) + 1
  if tol:
    assert stats['strides'] == [4, 4, 4] and nfe == 13
  torch.manual_seed(3)
  again, _ = fn(model)
  assert torch.equal(got, again) and fn.last_stats == stats, 'two runs under one seed differ'
  want = _by_hand(st, cfg, sde, model, eta, stats['strides'], torch.float64, 3, shape)
  own = _rel(_by_hand(st, cfg, sde, model, eta, stats['strides'], torch.float32, 3, shape), want)
  err = _rel(got, want)
  print(f'{family} eta {eta} tol {tol}: strides {stats["strides"]}; sampler deviates {err:.2e} from the float64 loop; the same '
        f'loop in torch fp32 deviates {own:.2e}: tolerance {4 * own:.2e}')
  assert err <= 4 * own


def test_window_one_is_the_sequential_sampler(st, hip_lib):
  """window = 1: twelve evaluations at batch B, and the noise of a stochastic run is what any window draws."""
  cfg, sde, model = _setup(st, hip_lib, 'vp')
  outs = {}
  for W in (1, 4):
    fn = sampler(st, cfg, sde, EPS, parallel_window=W, parallel_tol=0., parallel_eta=1.)
    torch.manual_seed(4)
    outs[W], nfe = fn(model)
    outs[W, 'rng'] = torch.cuda.get_rng_state()
    if W == 1:
      assert fn.last_stats['strides'] == [1] * STEPS and nfe == STEPS + 1
  assert torch.equal(outs[1, 'rng'], outs[4, 'rng'])
  print(f'window 4 at tol = 0 against window 1 on the tiny network: {_rel(outs[4], outs[1]):.2e}')


def test_class_conditional_sampler_under_guidance(st, hip_lib):
  """``with class_condition(model, y, 1.5): sampling_fn(model)``: a window is one evaluation at batch 2 W B."""
  mu = st.models.utils
  cfg = tiny_config(st, 'vp')
  cfg.model.num_classes = 3
  for k, v in dict(method='parallel', parallel_steps=STEPS, parallel_window=WINDOW, noise_removal=True).items():
    setattr(cfg.sampling, k, v)
  cfg.device = DEV
  sde = st.sde_lib.get_sde(cfg, None)
  torch.manual_seed(0)
  net = st.models.ncsnpp.NCSNpp(cfg, sde)
  net.set_backend(hip_lib)
  net = net.to(DEV)
  randomize_(net, 0)
  model = mu.DataParallel(net)
  net.engine().ensure_flat()
  model.eval()
  shape = shape_of(cfg)
  y = [2, 0]
  fn = sampler(st, cfg, sde, EPS, parallel_tol=1e30)
  batches = []
  inner = net._forward
  net._forward = lambda x, *a, **kw: batches.append(x.shape[0]) or inner(x, *a, **kw)
  try:
    with mu.class_condition(model, y, 1.5):
      saved = net._class_ctx
      torch.manual_seed(3)
      got, nfe = fn(model)
      assert net._class_ctx is saved
  finally:
    net._forward = inner
  assert batches == [2 * WINDOW * shape[0]] * 3 + [2 * shape[0]] and nfe == 13 and fn.last_stats['strides'] == [4, 4, 4]
  with mu.class_condition(model, y, 1.5):
    want = _by_hand(st, cfg, sde, model, 0., [4, 4, 4], torch.float64, 3, shape)
    own = _rel(_by_hand(st, cfg, sde, model, 0., [4, 4, 4], torch.float32, 3, shape), want)
  with mu.class_condition(model, [1, 1], 1.5):
    torch.manual_seed(3)
    other, _ = fn(model)
  err = _rel(got, want)
  print(f'class-conditional, guidance 1.5: sampler deviates {err:.2e} from the float64 loop, tolerance {4 * own:.2e}; other '
        f'classes move the result by {_rel(other, got):.2e}')
  assert err <= 4 * own
  assert not torch.equal(other, got), 'the classes did not reach the window'


@pytest.mark.parametrize('family', ['vp', 'wide'])
def test_fp16_runs(st, hip_lib, family):
  """precision = 'fp16' (the network only): runs, finite, the same counts.  Only the wide network has layers that take the
  fp16 forms."""
  cfg, sde, model = _setup(st, hip_lib, family)
  outs = {}
  for precision in ('fp32', 'fp16'):
    torch.manual_seed(9)
    outs[precision], nfe = sampler(st, cfg, sde, EPS, parallel_tol=1e30, precision=precision)(model)
    assert nfe == 13 and bool(torch.isfinite(outs[precision]).all())
  diff = float((outs['fp16'] - outs['fp32']).abs().max())
  print(f'{family}: fp16 against fp32: max |difference| {diff:.3e}')
  if family == 'wide':
    assert diff > 0, 'the fp16 mode did not reach the network'
