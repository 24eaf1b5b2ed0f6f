"""Dynamic thresholding in the DPM-Solver++ loop, dpm_solver.dynamic_threshold, and guidance rescale in the class-conditional
network, on the device (include/stk_guided.h).

The thresholded loop against float64 loops -- a closed-form score, and the tiny VP and VE networks -- with the measured
tolerance of tests/test_gpu_dpm_solver.py: the float64 reference loop is run again in fp32 (numpy for the closed-form score,
torch for the networks: every operation rounded), and four times its deviation from float64 is what the product loop may
deviate; the order statistic is 1-Lipschitz in max-norm, so the scheme carries over.  p = 0.9 and floor = 0.5 keep the
threshold active on most (step, sample) pairs, which the tests assert.  The deviations are printed.

The rescaled evaluation against the float64 formula applied to the engine's own halves c and u -- the same evaluation of
[x; x] with classes [y; null] the guided path makes, read through a context without guidance -- to 3 u |want|
(tests/_guided_ref.py).  Under grad mode the network itself may take other kernels than under no_grad, so that path is held
to the same bound against ITS own halves, and against the no_grad output directly where the halves of the two modes are the
same bits (printed)."""
import copy

import numpy as np
import pytest
import torch

import _dpm_ref as R
import _guided_ref as G
from _model_util import randomize_, tiny_config
from _sampler_util import setup, shape_of
from _stream_util import within

pytestmark = pytest.mark.gpu

EPS = 1e-3
P, FLOOR = 0.9, 0.5
STEPS = 10
f32 = lambda v: float(np.float32(v))


# ---- the loop with a closed-form score --------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gaussian_reference():
  """Per family: the start state (fp32), the float64 restatement's result and the same in numpy fp32.  Computed once."""
  out = {}
  for name, fam in (('vp', R.VP(0.1, 20.)), ('ve', R.VE(0.01, 50.))):
    gauss = G.WideGaussian((4, 3, 8, 8))
    x_T = gauss.prior(*fam.alpha_sigma(1.0)).astype(np.float32)
    s = R.schedule(fam, STEPS, order=2, skip='logsnr', eps=EPS, T=1.)
    a, sg = s['alpha'], s['sigma']
    res = {}
    for dtype in (np.float64, np.float32):
      mu, c2 = gauss.mu.astype(dtype), (gauss.c ** 2).astype(dtype)
      score = lambda x, i: -(x - dtype(a[i]) * mu) / (dtype(a[i] ** 2) * c2 + dtype(sg[i] ** 2))
      res[dtype] = G.sample(score, x_T, s, P, FLOOR, denoise=True, dtype=dtype)
    out[name] = dict(gauss=gauss, x_T=x_T, x64=res[np.float64][0], x32=res[np.float32][0], active=res[np.float64][1])
  return out


@pytest.mark.parametrize('family', ['vp', 've'])
def test_thresholded_loop_with_a_closed_form_score(st, hip_lib, gaussian_reference, family):
  dpm, S = st.dpm_solver, st.sde_lib
  dev = torch.device('cuda:0')
  sde = S.VPSDE(beta_min=0.1, beta_max=20) if family == 'vp' else S.VESDE(sigma_min=0.01, sigma_max=50)
  ref = gaussian_reference[family]
  assert ref['active'] > 0.5, f'thresholding active on {ref["active"]:.2f} of the (step, sample) pairs only'
  schedule = dpm.dpm_schedule(sde, STEPS, order=2, skip='logsnr', eps=EPS)
  mu = torch.from_numpy(ref['gauss'].mu.astype(np.float32)).to(dev)
  c2 = torch.from_numpy((ref['gauss'].c ** 2).astype(np.float32)).to(dev)
  index = {float(t): i for i, t in enumerate(schedule.times)}
  calls = []

  def score_fn(x, vec_t):
    i = index[float(vec_t[0])]
    calls.append(i)
    a, s = float(schedule.alpha[i]), float(schedule.sigma[i])
    return -(x - a * mu) / (c2 * (a * a) + s * s)

  x = torch.from_numpy(ref['x_T']).to(dev)
  out = dpm.dpm_sample(score_fn, x, schedule, denoise=True, threshold=(P, FLOOR))
  assert out is x and calls == list(range(STEPS + 1)), 'one evaluation per step and one at eps, the state advanced in place'
  got = out.cpu().double().numpy()
  assert float(np.abs(got).max()) <= 1.0, 'the thresholded data prediction at eps leaves [-1, 1]'
  own, dev_err = R.rel(ref['x32'], ref['x64']), R.rel(got, ref['x64'])
  print(f'{family}: thresholded product loop deviates {dev_err:.2e} from the float64 restatement; the restatement in numpy fp32 '
        f'deviates {own:.2e}: tolerance {4 * own:.2e}; threshold active on {ref["active"]:.2f} of the (step, sample) pairs')
  assert dev_err <= 4 * own
  # ... and it is another result than the plain loop's
  plain = dpm.dpm_sample(score_fn, torch.from_numpy(ref['x_T']).to(dev), schedule, denoise=True)
  assert R.rel(plain.cpu().double().numpy(), ref['x64']) > 1e-2


# ---- the sampler on the tiny networks -----------------------------------------------------------------------------------
def _setup(st, lib, family):
  """(cfg, sde, model, restated family) of a tiny network; the data of the copy of the config count as centred."""
  cfg, sde, model = setup(st, lib, family, dict(method='dpm_solver', dpm_steps=6, noise_removal=True))
  cfg = copy.deepcopy(cfg)
  cfg.data.centered = True
  fam = R.VE(sde.sigma_min, sde.sigma_max) if isinstance(sde, st.sde_lib.VESDE) else R.VP(sde.beta_0, sde.beta_1)
  return cfg, sde, model, fam


def _sampler(st, cfg, sde, **options):
  c = copy.deepcopy(cfg)
  for k, v in options.items():
    setattr(c.sampling, k, v)
  return st.sampling.get_sampling_fn(c, sde, shape_of(c), st.datasets.get_data_inverse_scaler(c), EPS)


def _by_hand(st, cfg, sde, model, fam, dtype, seed):
  """The test's own thresholded loop: the same engine score function, the update in torch `dtype` from the restatement's
  coefficients, the order statistic by a full sort -> (samples, fraction of (step, sample) pairs with the quantile above
  the floor)."""
  s = R.schedule(fam, STEPS, order=2, skip='logsnr', eps=EPS, T=1.)
  score_fn = st.models.utils.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
  torch.manual_seed(seed)
  active = []
  with torch.no_grad():
    x = sde.prior_sampling(shape_of(cfg)).to(cfg.device).to(dtype)
    rank = G.rank_of(P, x[0].numel())
    rows, times = list(s['coeffs']) + [s['final']], list(s['times'])
    d_prev = None
    for row, t in zip(rows, times):
      cx, cs, g, A, B = (float(v) if dtype == torch.float64 else f32(v) for v in row)
      vec_t = torch.ones(x.shape[0], device=x.device) * float(t)
      score = score_fn(x.float(), vec_t).to(dtype)
      d = cx * x + cs * score
      q = d.abs().reshape(x.shape[0], -1).sort(dim=1).values[:, rank]
      active.append((q > FLOOR).float().mean().item())
      sc = q.clamp_min(FLOOR).view(-1, 1, 1, 1)
      d = torch.minimum(torch.maximum(d, -sc), sc) / sc
      D = d if g == 0. else d + g * (d - d_prev)
      x, d_prev = A * x + B * D, d
    return st.datasets.get_data_inverse_scaler(cfg)(x), float(np.mean(active))


def _rel(a, b):
  return R.rel(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy())


@pytest.mark.parametrize('family', ['vp', 've'])
def test_thresholded_sampler_matches_a_float64_loop(st, hip_lib, family):
  cfg, sde, model, fam = _setup(st, hip_lib, family)
  fn = _sampler(st, cfg, sde, dpm_steps=STEPS, dpm_order=2, dpm_threshold=P, dpm_threshold_floor=FLOOR)
  torch.manual_seed(3)
  got, nfe = fn(model)
  assert nfe == STEPS + 1
  assert got.shape == shape_of(cfg) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
  assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0, 'a thresholded data prediction lies in [-1, 1]: [0, 1] after the scaler'
  torch.manual_seed(3)
  again, _ = fn(model)
  assert torch.equal(got, again), 'two runs under one seed differ'
  want, active = _by_hand(st, cfg, sde, model, fam, torch.float64, 3)
  own = _rel(_by_hand(st, cfg, sde, model, fam, torch.float32, 3)[0], want)
  err = _rel(got, want)
  print(f'{family}: thresholded sampler deviates {err:.2e} from the float64 loop; the same loop in torch fp32 deviates {own:.2e}: '
        f'tolerance {4 * own:.2e}; threshold active on {active:.2f} of the (step, sample) pairs')
  assert active > 0.5, 'the case does not exercise the threshold'
  assert err <= 4 * own
  torch.manual_seed(3)
  plain, _ = _sampler(st, cfg, sde, dpm_steps=STEPS, dpm_order=2)(model)
  assert not torch.equal(plain, got)


@pytest.mark.parametrize('family', ['vp', 've'])
def test_without_a_threshold_the_sampler_is_the_parents(st, hip_lib, family, monkeypatch):
  """The keys absent: no entry of stk_guided.h is called, and the result is, bit for bit, the loop of one score evaluation
  and one stk_dpm_update_f32 per step."""
  cfg, sde, model, _ = _setup(st, hip_lib, family)
  dpm = st.dpm_solver
  assert dpm.threshold_options(cfg) is None

  def refuse(*a):
    raise AssertionError('an entry of include/stk_guided.h was called without a threshold')

  for name in st.engine.lib.SIGNATURES_GUIDED:
    monkeypatch.setattr(hip_lib, name[4:], refuse)
  torch.manual_seed(11)
  got, nfe = _sampler(st, cfg, sde, dpm_order=2)(model)
  assert nfe == 7
  schedule = dpm.dpm_schedule(sde, 6, order=2, skip='logsnr', eps=EPS)
  torch.manual_seed(11)
  with st.models.utils.sampling_run(model, 'fp32'):
    score_fn = st.models.utils.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
    x = sde.prior_sampling(shape_of(cfg)).to(cfg.device).contiguous()
    hist = torch.empty_like(x)
    rows, times = list(schedule.coeffs) + [schedule.final], list(schedule.times)
    inf = float('inf')
    for row, t in zip(rows, times):
      score = score_fn(x, torch.ones(x.shape[0], device=x.device) * float(t)).contiguous()
      cx, cs, g, A, B = (float(v) for v in row)
      hip_lib.dpm_update_f32(x.data_ptr(), score.data_ptr(), hist.data_ptr() if g != 0. else None, cx, cs, g, A, B, -inf, inf,
                             x.data_ptr(), hist.data_ptr(), x.numel(), torch.cuda.current_stream().cuda_stream)
    want = st.datasets.get_data_inverse_scaler(cfg)(x)
  assert torch.equal(got, want)


def _same(got, want):
  """The same bits, a NaN standing for any NaN (a quotient's NaN payload is the hardware's)."""
  nan = np.isnan(want)
  return np.array_equal(np.isnan(got), nan) and np.array_equal(G.bits(got)[~nan], G.bits(want)[~nan])


def test_dynamic_threshold_matches_its_restatement(st, hip_lib):
  dpm = st.dpm_solver
  dev = torch.device('cuda:0')
  rng = np.random.RandomState(5)
  x0 = (rng.standard_normal((4, 3, 8, 8)) * np.array([0.2, 1.0, 2.0, 4.0]).reshape(4, 1, 1, 1)).astype(np.float32)
  x0[3, 1, 2, 3] = np.float32('nan')
  flat = x0.reshape(4, -1)
  for p, floor in ((0.9, 0.5), (0.995, 1.0), (1.0, 1.0), (0.5, 3.0)):
    xd = torch.from_numpy(x0).to(dev)
    out, s = dpm.dynamic_threshold(xd, p, floor)
    q = G.select(flat, G.rank_of(p, flat.shape[1]))
    want_s = G.scale_of(q, floor)
    assert out.shape == xd.shape and s.shape == (4,) and out.data_ptr() != xd.data_ptr()
    assert _same(s.cpu().numpy(), want_s), (p, floor)
    assert _same(out.cpu().numpy().reshape(4, -1), G.threshold(flat, want_s)), (p, floor)
    assert np.array_equal(G.bits(xd.cpu().numpy()), G.bits(x0)), 'the operand was written'
    assert bool(np.isnan(want_s[3])) == (G.rank_of(p, flat.shape[1]) == flat.shape[1] - 1), 'the NaN counts only at the top rank'
  assert float(np.nanmax(np.abs(out.cpu().numpy()))) <= 1.0


# ---- guidance rescale in the class-conditional network ---------------------------------------------------------------------------
C = 3
_built = {}


def _class_model(st, lib):
  if 'vp' not in _built:
    cfg = tiny_config(st, 'vp')
    cfg.model.num_classes = C
    cfg.device = torch.device('cuda:0')
    sde = st.sde_lib.get_sde(cfg, None)
    torch.manual_seed(0)
    net = st.models.ncsnpp.NCSNpp(cfg, sde)
    net.set_backend(lib)
    net = net.to(cfg.device)
    randomize_(net, 0)
    model = st.models.utils.DataParallel(net)
    net.engine().ensure_flat()
    model.eval()
    _built['vp'] = (cfg, sde, model)
  return _built['vp']


def _halves(mu, model, x, cond, y):
  """(c, u) of the evaluation of [x; x] with classes [y; null] that the guided path makes: through a context without guidance."""
  B = x.shape[0]
  with mu.class_condition(model, list(y) + [None] * B):
    out = model(torch.cat([x, x]), torch.cat([cond, cond]))
  return out[:B], out[B:]


def _rows(t):
  return t.detach().cpu().numpy().reshape(t.shape[0], -1)


def test_rescaled_guidance(st, hip_lib):
  mu = st.models.utils
  cfg, sde, model = _class_model(st, hip_lib)
  dev = cfg.device
  g = torch.Generator().manual_seed(1)
  x = torch.randn(3, cfg.data.num_channels, cfg.data.image_size, cfg.data.image_size, generator=g).to(dev)
  cond = ((torch.rand(3, generator=g) * 0.9 + 0.05) * 999).to(dev)
  y = [2, 0, 1]
  w, phi = 2.0, f32(0.7)
  inner = model.module
  with torch.no_grad():
    c, u = _halves(mu, model, x, cond, y)
    with mu.class_condition(model, y, w):
      today = model(x, cond)
    with mu.class_condition(model, y, w, rescale=0.0):
      assert torch.equal(model(x, cond), today), 'rescale = 0 is not today\'s path'
    comb = torch.empty_like(today)
    hip_lib.cfg_combine_f32(c.contiguous().data_ptr(), u.contiguous().data_ptr(), w, comb.data_ptr(), comb.numel(),
                            torch.cuda.current_stream().cuda_stream)
    assert torch.equal(today, comb), 'the halves read through the context are not the guided path\'s'
    with mu.class_condition(model, y, w, rescale=phi):
      assert inner._cfg_rescale == phi
      got = model(x, cond)
      again = model(x, cond)
      with mu.class_condition(model, y, w):                     # contexts nest and restore the rescale
        assert inner._cfg_rescale == 0.0 and torch.equal(model(x, cond), today)
      assert inner._cfg_rescale == phi
    assert inner._cfg_rescale == 0.0 and inner._class_ctx is None
    assert torch.equal(got, again)
    with mu.class_condition(model, y, 0.0, rescale=phi):        # accepted, and does nothing
      plain = model(x, cond)
    with mu.class_condition(model, y):
      assert torch.equal(model(x, cond), plain)
  want, _, f = G.rescale64(_rows(c), _rows(u), w, phi)
  assert bool(np.all(np.abs(f - 1.0) > 1e-3)), f'the factors {f} leave the case without a rescale'
  worst = within(got.reshape(3, -1), want, np.abs(want), G.K_RESCALE, 'rescaled guidance (no_grad)')
  print(f'rescaled guidance: factors {f}, no_grad worst {worst:.2f} u |want| (bound {G.K_RESCALE})')
  # grad mode: the same formula by torch operators
  xg = x.clone().requires_grad_(True)
  with mu.class_condition(model, y, w, rescale=phi):
    out = model(xg, cond)
  cg, ug = _halves(mu, model, x.clone().requires_grad_(True), cond, y)
  want_g, _, _ = G.rescale64(_rows(cg), _rows(ug), w, phi)
  worst_g = within(out.reshape(3, -1), want_g, np.abs(want_g), G.K_RESCALE, 'rescaled guidance (grad mode)')
  same = torch.equal(cg.detach(), c) and torch.equal(ug.detach(), u)
  print(f'rescaled guidance: grad mode worst {worst_g:.2f} u |want|; its halves are {"" if same else "NOT "}the bits of the '
        f'no_grad halves')
  if same:
    within(out.reshape(3, -1), got.reshape(3, -1).cpu().double(), got.reshape(3, -1).cpu().double().abs(), G.K_RESCALE,
           'grad mode against no_grad')
  # ... which autograd differentiates: the gradient is not the unrescaled combination's
  go = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(dev)
  gx, = torch.autograd.grad((out * go).sum(), xg)
  xs = x.clone().requires_grad_(True)
  with mu.class_condition(model, y, w):
    g0, = torch.autograd.grad((model(xs, cond) * go).sum(), xs)
  assert bool(torch.isfinite(gx).all()) and _rel(gx, g0) > 1e-3


def test_guidance_rescale_and_threshold_together(st, hip_lib):
  mu = st.models.utils
  cfg, sde, model = _class_model(st, hip_lib)
  c = copy.deepcopy(cfg)
  for k, v in dict(method='dpm_solver', dpm_steps=4, dpm_order=2, noise_removal=True, dpm_threshold=0.9, dpm_threshold_floor=0.5).items():
    setattr(c.sampling, k, v)
  assert c.data.centered
  fn = st.sampling.get_sampling_fn(c, sde, shape_of(c), st.datasets.get_data_inverse_scaler(c), EPS)

  def run(*context):
    torch.manual_seed(3)
    with mu.class_condition(model, *context):
      return fn(model)

  got, nfe = run([0, 2], 2.0, 0.7)
  assert nfe == 5 and got.shape == shape_of(c) and bool(torch.isfinite(got).all())
  assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
  assert torch.equal(run([0, 2], 2.0, 0.7)[0], got), 'two runs under one seed differ'
  assert not torch.equal(run([0, 2], 2.0)[0], got), 'the rescale does not reach the sampler'
