"""stk_dpm_update_f32 (include/stk_solver.h, csrc/solver.hip) and the DPM-Solver++ sampler built on it, on the device.

The kernel against float64.  The bound is the rounding model of the header's five operations, not a blanket tolerance:
every output element is an expression of rounded products and sums, and standard forward analysis bounds its error by
gamma_k B, where B is the same expression on absolute values and k the number of roundings on the longest path from an
operand to the result, gamma_k = k u / (1 - k u), u = 2^-24.  For d that path is (product, sum): k = 2; for x_out it is
(product, sum -> d, d - d_prev, times g, + d -> D, times B, + A x): k = 7.  A fused multiply-add only removes roundings.
The clamp rounds nothing and is 1-Lipschitz, and with clip_lo <= 0 <= clip_hi it only shrinks |d|, so the unclamped B
stays a bound.  The coefficients reach the reference as the fp32 values the kernel receives.  The test holds K_D = 3 and
K_X = 8 (gamma_2 < 3 u, gamma_7 < 8 u), with
  B_d = |cx| |x| + |cs| |score|,   B_D = B_d + |g| (B_d + |d_prev|),   B_x = |A| |x| + |B| B_D.

The loop with a closed-form score, and the sampler on the tiny networks, against float64 loops: the tolerance is measured,
not fixed in advance -- the float64 reference loop is run again in fp32 (numpy for the closed-form score, torch for the
networks: every operation rounded), and four times its deviation from float64 is what the product loop may deviate.  The
deviations are printed by the tests.  On the CPU the restatement in numpy fp32 deviates from float64 by 3.6e-7 (VP) and
9.3e-7 (VE) relative at order 2, 20 steps; the figures of the product loop on an MI355X are not recorded yet (MEASURED).
"""
import itertools

import numpy as np
import pytest
import torch

import _dpm_ref as R
from _sampler_util import sampler, setup, shape_of as _shape
from _stream_util import case_id, place, within

pytestmark = pytest.mark.gpu

MEASURED = "unmeasured: no MI355X run of this file has been recorded"

K_D, K_X = 3, 8
EPS = 1e-3
FLT_MAX = float(np.finfo(np.float32).max)
INF = float('inf')
f32 = lambda v: float(np.float32(v))
ROW = tuple(f32(v) for v in (1.3, 0.7, 0.45, 0.8, 0.35))          # (cx, cs, g, A, B): a second-order step
CLIPS = {'off': None, 'on': (-1., 1.), 'inf': (-INF, INF)}
# vector path; n = 315, scalar path; one element; a 16-byte-aligned buffer entered one element in (scalar path);
# 3072 blocks of vector items against stk_ew_grid's cap of 2048 (common.h: 8 blocks per CU, 256 CUs): the grid strides;
# the same entered one element in: 3145728 scalar items against 2048 x 256 threads, the scalar grid strides too
SHAPES = [((2, 3, 8, 8), False), ((3, 3, 5, 7), False), ((1, 1, 1, 1), False), ((2, 3, 8, 8), True),
          ((16, 3, 256, 256), False), ((16, 3, 256, 256), True)]


def _launch(lib, x, score, d_prev, row, clip, x_out, d_out):
  lo, hi = (-INF, INF) if clip is None else clip
  ptr = lambda t: None if t is None else t.data_ptr()
  lib.dpm_update_f32(x.data_ptr(), score.data_ptr(), ptr(d_prev), *row, lo, hi, x_out.data_ptr(), ptr(d_out), x.numel(),
                     torch.cuda.current_stream().cuda_stream)


def _restate(x, score, d_prev, row, clip):
  """The header's five lines on float64 tensors -> (x_out, d, B_x, B_d)."""
  cx, cs, g, A, B = row
  d = cx * x + cs * score
  if clip is not None:
    d = torch.clamp(d, clip[0], clip[1])
  D = d if d_prev is None else d + g * (d - d_prev)
  b_d = abs(cx) * x.abs() + abs(cs) * score.abs()
  b_D = b_d if d_prev is None else b_d + abs(g) * (b_d + d_prev.abs())
  return A * x + B * D, d, abs(A) * x.abs() + abs(B) * b_D, b_d


@pytest.fixture(scope='module')
def operands():
  """x, score, d_prev per shape, float32 on the host, and their float64 copies: drawn once."""
  out = {}
  for shape in sorted({s for s, _ in SHAPES}):
    g = torch.Generator().manual_seed(sum(shape))
    t = [torch.randn(shape, generator=g) * scale for scale in (1.5, 2.0, 1.0)]
    out[shape] = (t, [v.double() for v in t])
  return out


@pytest.mark.parametrize('shape,shifted', SHAPES, ids=case_id)
def test_kernel_matches_float64(hip_lib, operands, shape, shifted):
  dev = torch.device('cuda:0')
  (x, s, p), (x64, s64, p64) = operands[shape]
  xd, sd, pd = (place(t, dev, shifted) for t in (x, s, p))
  worst_x = worst_d = 0.0
  for use_prev, use_dout in itertools.product((True, False), (True, False)):
    row = ROW if use_prev else ROW[:2] + (0.,) + ROW[3:]
    outs = {}
    for name, clip in CLIPS.items():
      want_x, want_d, b_x, b_d = _restate(x64, s64, p64 if use_prev else None, row, clip)
      x_out = place(torch.full(shape, float('nan')), dev, shifted)
      d_out = place(torch.full(shape, float('nan')), dev, shifted) if use_dout else None
      _launch(hip_lib, xd, sd, pd if use_prev else None, row, clip, x_out, d_out)
      what = f'dpm_update {shape} shifted={shifted} d_prev={use_prev} d_out={use_dout} clip={name}'
      worst_x = max(worst_x, within(x_out, want_x, b_x, K_X, what + ' x_out'))
      if use_dout:
        worst_d = max(worst_d, within(d_out, want_d, b_d, K_D, what + ' d_out'))
        if clip is not None:
          assert float(d_out.min()) >= clip[0] and float(d_out.max()) <= clip[1]
      outs[name] = (x_out, d_out)
      # state and history kept in place: bit-identical to the separate-buffer form
      xa, pa = place(x, dev, shifted), place(p, dev, shifted)
      _launch(hip_lib, xa, sd, pa if use_prev else None, row, clip, xa, pa if (use_prev and use_dout) else d_out)
      assert torch.equal(xa, x_out), what + ': x_out = x differs from the separate-buffer form'
      if use_prev and use_dout:
        assert torch.equal(pa, d_out), what + ': d_out = d_prev differs from the separate-buffer form'
    # bounds of -inf / +inf leave every finite d bit-identical: the same bits as bounds no fp32 number reaches
    x_max, d_max = place(torch.full(shape, float('nan')), dev, shifted), place(torch.full(shape, float('nan')), dev, shifted)
    _launch(hip_lib, xd, sd, pd if use_prev else None, row, (-FLT_MAX, FLT_MAX), x_max, d_max)
    for name in ('off', 'inf'):
      assert torch.equal(outs[name][0], x_max), f'{shape}: clip {name} is not bit-identical to an unreachable clip'
      if use_dout:
        assert torch.equal(outs[name][1], d_max)
    assert torch.equal(outs['off'][0], outs['inf'][0])
    if bool(((row[0] * x64 + row[1] * s64).abs() > 1.001).any()):          # the one-element case may lie inside the bounds
      assert not torch.equal(outs['on'][0], outs['off'][0]), 'the clamp changed nothing'
  assert torch.equal(xd.cpu(), x) and torch.equal(sd.cpu(), s) and torch.equal(pd.cpu(), p), 'an operand was written'
  print(f'dpm_update {shape} shifted={shifted}: worst x_out {worst_x:.2f} u B (bound {K_X}), worst d_out {worst_d:.2f} u B (bound {K_D})')


def test_package_update_passes_the_clip(st, hip_lib):
  """dpm_solver._update, the launch the loop makes: clip=None is the entry's -inf / +inf."""
  dpm = st.dpm_solver
  dev = torch.device('cuda:0')
  g = torch.Generator().manual_seed(2)
  x, s = (torch.randn(2, 3, 8, 8, generator=g).to(dev) * 2 for _ in range(2))
  outs = []
  for clip in (None, (-INF, INF), (-0.25, 0.5)):
    x_out, d_out = torch.empty_like(x), torch.empty_like(x)
    dpm._update(hip_lib, x, s, None, ROW[:2] + (0.,) + ROW[3:], dpm._clip_bounds(clip), x_out, d_out)
    outs.append((x_out, d_out))
  assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
  assert float(outs[2][1].min()) == -0.25 and float(outs[2][1].max()) == 0.5
  assert torch.equal(outs[2][1], torch.clamp(outs[0][1], -0.25, 0.5))


def test_return_codes_and_nothing_written(hip_lib):
  """Every refusal returns before any launch: the outputs keep their sentinel."""
  dev = torch.device('cuda:0')
  raw = hip_lib.dpm_update_f32.raw
  x, s, p = (torch.randn(2, 3, 4, 4, device=dev) for _ in range(3))
  x_out, d_out = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
  n = x.numel()
  stream = torch.cuda.current_stream().cuda_stream
  nan = float('nan')
  sentinels = (x_out, d_out)

  def rc(x=x, s=s, p=p, g=0.45, lo=-INF, hi=INF, x_out=x_out, d_out=d_out, n=n):
    ptr = lambda t: None if t is None else t.data_ptr()
    code = raw(ptr(x), ptr(s), ptr(p), 1.3, 0.7, g, 0.8, 0.35, lo, hi, ptr(x_out), ptr(d_out), n, stream)
    torch.cuda.synchronize()
    assert bool((sentinels[0] == 7.0).all()) and bool((sentinels[1] == 7.0).all()), 'a refused call wrote'
    return code

  EINVAL, EUNSUPPORTED = -1, -3
  assert rc(x=None) == EINVAL
  assert rc(s=None) == EINVAL
  assert rc(x_out=None) == EINVAL
  assert rc(n=0) == EINVAL
  assert rc(n=-4) == EINVAL
  assert rc(p=None, g=0.45) == EINVAL                    # a second-order step without history
  assert rc(p=None, g=-0.1) == EINVAL
  assert rc(lo=1., hi=-1.) == EINVAL
  assert rc(lo=INF, hi=-INF) == EINVAL
  assert rc(lo=nan, hi=1.) == EINVAL and rc(lo=-1., hi=nan) == EINVAL
  assert rc(n=2 ** 31) == EUNSUPPORTED
  assert rc(n=2 ** 31 + 4) == EUNSUPPORTED
  assert rc(n=2 ** 40) == EUNSUPPORTED
  # ... and the accepted edge forms run: no history with g == 0, no d_out, equal bounds
  assert rc(p=None, g=0., x_out=torch.empty_like(x), d_out=None) == 0
  assert rc(lo=0.5, hi=0.5, x_out=torch.empty_like(x), d_out=None) == 0
  # the checked binding raises the package's error
  with pytest.raises(RuntimeError, match='stk_dpm_update_f32 failed'):
    hip_lib.dpm_update_f32(x.data_ptr(), s.data_ptr(), None, 1.3, 0.7, 0.45, 0.8, 0.35, -INF, INF, x_out.data_ptr(), None, n, stream)


# ---- the loop with a closed-form score --------------------------------------------------------------------------------
def _families(st):
  S = st.sde_lib
  return {'vp': (S.VPSDE(beta_min=0.1, beta_max=20), R.VP(0.1, 20.)), 've': (S.VESDE(sigma_min=0.01, sigma_max=50), R.VE(0.01, 50.))}


@pytest.fixture(scope='module')
def gaussian_reference():
  """Per family and order: the start state (fp32), the float64 restatement's result, the same in numpy fp32, the exact
  flow.  Computed once."""
  out = {}
  for name, fam in (('vp', R.VP(0.1, 20.)), ('ve', R.VE(0.01, 50.))):
    gauss = R.Gaussian((4, 3, 8, 8))
    x_T = gauss.prior(*fam.alpha_sigma(1.0)).astype(np.float32)
    for order in (1, 2):
      x64, flow = R.gaussian_run(fam, gauss, 20, order, eps=EPS, x_T=x_T)
      x32, _ = R.gaussian_run(fam, gauss, 20, order, dtype=np.float32, eps=EPS, x_T=x_T)
      out[name, order] = dict(gauss=gauss, x_T=x_T, x64=x64, x32=x32, flow=flow)
  return out


@pytest.mark.parametrize('family', ['vp', 've'])
def test_loop_with_a_closed_form_score(st, hip_lib, gaussian_reference, family):
  dpm = st.dpm_solver
  dev = torch.device('cuda:0')
  sde, _ = _families(st)[family]
  errs = {}
  for order in (1, 2):
    ref = gaussian_reference[family, order]
    schedule = dpm.dpm_schedule(sde, 20, order=order, skip='logsnr', eps=EPS)
    mu = torch.from_numpy(ref['gauss'].mu.astype(np.float32)).to(dev)
    c2 = torch.from_numpy((ref['gauss'].c ** 2).astype(np.float32)).to(dev)
    index = {float(t): i for i, t in enumerate(schedule.times)}
    calls = []

    def score_fn(x, vec_t):
      assert vec_t.shape == (4,) and vec_t.dtype == torch.float32 and vec_t.device == x.device
      i = index[float(vec_t[0])]                    # the loop hands over exactly the schedule's fp32 times
      assert bool((vec_t == vec_t[0]).all())
      calls.append(i)
      a, s = float(schedule.alpha[i]), float(schedule.sigma[i])
      return -(x - a * mu) / (c2 * (a * a) + s * s)

    x = torch.from_numpy(ref['x_T']).to(dev)
    out = dpm.dpm_sample(score_fn, x, schedule)
    assert out is x and calls == list(range(20)), 'one evaluation per step, the state advanced in place'
    got = out.cpu().double().numpy()
    own = R.rel(ref['x32'], ref['x64'])               # what fp32 arithmetic alone does to the restatement
    dev_err = R.rel(got, ref['x64'])
    errs[order] = R.rel(got, ref['flow'])
    print(f'{family} order {order}: product loop deviates {dev_err:.2e} from the float64 restatement; the restatement in numpy '
          f'fp32 deviates {own:.2e}: tolerance {4 * own:.2e}; error against the exact flow {errs[order]:.3e}')
    assert dev_err <= 4 * own
  # second order lies closer to the exact flow than first order, by at least the factor 3.5 the CPU convergence test
  # asserts of one doubling of the steps (the restatement itself: 8.6 for VP and 9.6 for VE at 20 steps)
  print(f'{family}: order-1 error / order-2 error = {errs[1] / errs[2]:.2f}')
  assert errs[1] / errs[2] >= 3.5
  assert errs[2] <= 2e-2                              # ... and is what the restatement gives: 1.2e-2 (VP), 9.7e-3 (VE)


# ---- the sampler on the tiny networks -----------------------------------------------------------------------------------
def _setup(st, lib, family):
  """(cfg, sde, model, restated family) of a tiny network."""
  cfg, sde, model = setup(st, lib, family, dict(method='dpm_solver', dpm_steps=6, noise_removal=True))
  fam = R.VE(sde.sigma_min, sde.sigma_max) if isinstance(sde, st.sde_lib.VESDE) else R.VP(sde.beta_0, sde.beta_1)
  return cfg, sde, model, fam


def _sampler(st, cfg, sde, **options):
  return sampler(st, cfg, sde, EPS, **options)


def _by_hand(st, cfg, sde, model, fam, order, denoise, dtype, seed, clip=None):
  """The test's own loop: the same engine score function, the update in torch `dtype` from the restatement's coefficients."""
  s = R.schedule(fam, 6, order=order, skip='logsnr', eps=EPS, T=1.)
  score_fn = st.models.utils.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
  torch.manual_seed(seed)
  with torch.no_grad():
    x = sde.prior_sampling(_shape(cfg)).to(cfg.device).to(dtype)
    rows = list(s['coeffs']) + ([s['final']] if denoise else [])
    times = list(s['times'][:-1]) + ([s['times'][-1]] if denoise else [])
    d_prev = None
    for row, t in zip(rows, times):
      cx, cs, g, A, B = (float(v) if dtype == torch.float64 else f32(v) for v in row)
      vec_t = torch.ones(x.shape[0], device=x.device) * float(t)
      score = score_fn(x.float(), vec_t).to(dtype)
      d = cx * x + cs * score
      if clip is not None:
        d = torch.clamp(d, clip[0], clip[1])
      D = d if g == 0. else d + g * (d - d_prev)
      x, d_prev = A * x + B * D, d
    return st.datasets.get_data_inverse_scaler(cfg)(x)


def _rel(a, b):
  return R.rel(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy())


@pytest.mark.parametrize('denoise', [True, False], ids=['denoise', 'state'])
@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('family', ['vp', 've'])
def test_sampler_matches_a_float64_loop(st, hip_lib, family, order, denoise):
  cfg, sde, model, fam = _setup(st, hip_lib, family)
  fn = _sampler(st, cfg, sde, dpm_order=order, noise_removal=denoise)
  torch.manual_seed(3)
  got, nfe = fn(model)
  assert nfe == (7 if denoise else 6)
  assert got.shape == _shape(cfg) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
  torch.manual_seed(3)
  again, _ = fn(model)
  assert torch.equal(got, again), 'two runs under one seed differ'
  want = _by_hand(st, cfg, sde, model, fam, order, denoise, torch.float64, 3)
  own = _rel(_by_hand(st, cfg, sde, model, fam, order, denoise, torch.float32, 3), want)
  err = _rel(got, want)
  print(f'{family} order {order} denoise={denoise}: sampler deviates {err:.2e} from the float64 loop; the same loop in torch fp32 '
        f'deviates {own:.2e}: tolerance {4 * own:.2e}')
  assert err <= 4 * own


@pytest.mark.parametrize('family', ['vp', 've'])
def test_orders_and_denoising_differ(st, hip_lib, family):
  """The options reach the loop: the two orders, and the state against the data prediction, are different tensors."""
  cfg, sde, model, _ = _setup(st, hip_lib, family)
  outs = {}
  for order, denoise in itertools.product((1, 2), (True, False)):
    torch.manual_seed(3)
    outs[order, denoise], _ = _sampler(st, cfg, sde, dpm_order=order, noise_removal=denoise)(model)
  assert not torch.equal(outs[1, True], outs[2, True]) and not torch.equal(outs[1, False], outs[2, False])
  assert not torch.equal(outs[2, True], outs[2, False])


@pytest.mark.parametrize('family', ['vp', 've'])
def test_the_only_draw_is_the_prior(st, hip_lib, family):
  """The generators after a whole run are where one sde.prior_sampling(shape) alone leaves them."""
  cfg, sde, model, _ = _setup(st, hip_lib, family)
  fn = _sampler(st, cfg, sde, dpm_order=2)
  torch.manual_seed(5)
  fn(model)
  after_run = (torch.get_rng_state(), torch.cuda.get_rng_state())
  torch.manual_seed(5)
  sde.prior_sampling(_shape(cfg))
  after_prior = (torch.get_rng_state(), torch.cuda.get_rng_state())
  torch.manual_seed(5)
  untouched = (torch.get_rng_state(), torch.cuda.get_rng_state())
  assert torch.equal(after_run[0], after_prior[0]) and torch.equal(after_run[1], after_prior[1])
  assert not (torch.equal(after_prior[0], untouched[0]) and torch.equal(after_prior[1], untouched[1])), 'the prior drew nothing'


@pytest.mark.parametrize('family', ['vp', 've'])
def test_clip_keeps_the_data_prediction_in_range(st, hip_lib, family):
  cfg, sde, model, fam = _setup(st, hip_lib, family)
  torch.manual_seed(7)
  free, _ = _sampler(st, cfg, sde, dpm_order=2)(model)
  torch.manual_seed(7)
  got, nfe = _sampler(st, cfg, sde, dpm_order=2, dpm_clip=(-1., 1.))(model)
  assert nfe == 7
  inv = st.datasets.get_data_inverse_scaler(cfg)
  lo, hi = float(inv(torch.tensor(-1.))), float(inv(torch.tensor(1.)))
  print(f'{family}: unclipped data prediction in [{float(free.min()):.3f}, {float(free.max()):.3f}] after the inverse scaler, '
        f'clipped in [{float(got.min()):.3f}, {float(got.max()):.3f}], range [{lo}, {hi}]')
  assert float(got.min()) >= lo and float(got.max()) <= hi
  assert float(free.min()) < lo or float(free.max()) > hi, 'the case does not exercise the clamp'
  want = _by_hand(st, cfg, sde, model, fam, 2, True, torch.float64, 7, clip=(-1., 1.))
  own = _rel(_by_hand(st, cfg, sde, model, fam, 2, True, torch.float32, 7, clip=(-1., 1.)), want)
  print(f'{family} clipped: sampler deviates {_rel(got, want):.2e} from the float64 loop, tolerance {4 * own:.2e}')
  assert _rel(got, want) <= 4 * own


@pytest.mark.parametrize('family', ['vp', 've', 'wide'])
def test_fp16_runs(st, hip_lib, family):
  """precision = 'fp16' (the network only): runs, finite, the same nfe.  No threshold on the difference from fp32: sample
  quality in that mode is unmeasured everywhere in this project.  Only the wide network has layers that take the fp16 forms."""
  cfg, sde, model, _ = _setup(st, hip_lib, family)
  outs = {}
  for precision in ('fp32', 'fp16'):
    torch.manual_seed(9)
    outs[precision], nfe = _sampler(st, cfg, sde, dpm_order=2, precision=precision)(model)
    assert nfe == 7 and bool(torch.isfinite(outs[precision]).all())
  diff = float((outs['fp16'] - outs['fp32']).abs().max())
  print(f'{family}: fp16 against fp32 after 7 evaluations: max |difference| {diff:.3e} (samples within '
        f'[{float(outs["fp32"].min()):.3f}, {float(outs["fp32"].max()):.3f}])')
  if family == 'wide':
    assert diff > 0, 'the fp16 mode did not reach the network'
