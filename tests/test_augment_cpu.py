"""Host side of the non-leaky augmentation (augment.py, models/ncsnpp.py, models/utils.py augment_condition,
losses.get_step_fn): the float64 restatement of the operator against cases that can be checked by hand, the float32 copy of
it inside the bound of the GPU test, the draws of the pipe, every ValueError, the refusal of the embedding on the checker and
the ctypes table of include/stk_augment.h.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import _augment_ref as R
from _model_util import tiny_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = {'box2': R.box_filter(2), 'tent4': R.tent4(), 'kaiser12': R.default_filter()}
SHAPES = [(8, 8), (8, 12), (32, 32), (64, 64)]


# ---- the reference against hand-checkable cases ------------------------------------------------------------------------------
@pytest.mark.parametrize('fname', list(FILTERS))
def test_a_constant_plane_stays_constant(fname):
  f = FILTERS[fname]
  S = np.full((8, 12), 0.75)
  for name, p in R.rows(8, 12).items():
    O = R.warp(S, p, f)
    assert np.abs(O - 0.75).max() <= 1e-6, name       # the fp32 taps sum to 1 within rounding; the two phases to 1/2 each


@pytest.mark.parametrize('fname', list(FILTERS))
def test_identity_map_is_down_of_up_and_commutes_with_flips(fname):
  """A = I through the filters (a translation of one whole period 2(W - 1) keeps the row off the exact path): Down(Up(S)),
  computed here directly from the definition with explicit index arithmetic; flipping the input flips that output."""
  f = FILTERS[fname].astype(np.float64)
  T, h = len(f), len(f) // 2
  H, W = 8, 12
  S = R.image(1, 1, H, W, seed=3)[0, 0].astype(np.float64)

  def refl(i, n):
    m = i % (2 * n - 2)
    return m if m < n else 2 * n - 2 - m

  def up1(v):                         # U[j] for every j the down pass reads, as a dict
    n = len(v)
    out = {}
    for j in range(-(h - 1), 2 * n + h - 1):
      acc = 0.0
      for k in range(T):
        m = j + h - 1 - k
        if m % 2 == 0:
          acc += f[k] * v[refl(m // 2, n)]
      out[j] = 2 * acc
    return out

  def down_up_axis(a):                # along the last axis
    n = a.shape[-1]
    res = np.zeros_like(a)
    for r in range(a.shape[0]):
      U = up1(a[r])
      for i in range(n):
        res[r, i] = sum(f[k] * U[2 * i + k - (h - 1)] for k in range(T))
    return res

  want = down_up_axis(down_up_axis(S).T).T
  period = R.row(shift=(-2.0 * (W - 1), 0.0))
  assert not R.is_identity(period)
  got = R.warp(S, period, FILTERS[fname])
  assert np.abs(got - want).max() <= 1e-13
  for fx, fy in ((1, 0), (0, 1), (1, 1)):
    p = period.copy()
    p[0], p[1] = fx, fy
    flipped = want[::-1] if fy else want
    flipped = flipped[:, ::-1] if fx else flipped
    assert np.abs(R.warp(S, p, FILTERS[fname]) - flipped).max() <= 1e-13, (fx, fy)
  # the exact path: the flipped input itself
  assert np.array_equal(R.warp(S, R.row(fx=1), FILTERS[fname]), S[:, ::-1])


def test_an_integer_shift_commutes_with_the_operator_up_to_reflection():
  """Shifting by d whole pixels: the output is Down(Up(.)) of the reflect-extended plane read d pixels away, so away from the
  border (further than d plus the filters' reach) it is the unshifted output moved by d."""
  f = R.default_filter()
  H = W = 32
  S = R.image(1, 1, H, W, seed=5)[0, 0].astype(np.float64)
  base = R.warp(S, R.row(shift=(-2.0 * (W - 1), 0.0)), f)          # A = I through the filters
  d = 3
  got = R.warp(S, R.row(shift=(float(d), 0.0)), f)                   # the image moves d pixels to the right
  assert np.abs(got[:, d:] - base[:, :W - d]).max() <= 1e-13
  # and the d columns that enter at the border are those of the reflection: Down(Up(.)) of the explicitly reflect-padded
  # plane (16 pixels, beyond the 6 the filters reach), read d pixels to the left of the plane's own columns
  pad = 16
  big = np.pad(S, pad, mode='reflect')
  ref_big = R.warp(big, R.row(shift=(-2.0 * (W + 2 * pad - 1), 0.0)), f)
  assert np.abs(got - ref_big[pad:pad + H, pad - d:pad + W - d]).max() <= 1e-13
  assert np.abs(got[:, :d] - base[:, :d]).max() > 1e-3              # ... which the unshifted output does not hold


def test_the_reduced_translation_is_exact_and_in_range():
  for n in (8, 12, 32, 64):
    for t in (0.0, 0.3, -0.3, n - 1.0, n - 0.5, -(n - 0.5), 3.0 * n + 0.3, -3.0 * n - 0.7, 1e6 + 0.25, -7e5):
      t32 = np.float32(t)
      r = R.reduced_translation(t32, n)
      assert abs(float(r)) <= n - 1
      k = (float(t32) - float(r)) / (2 * n - 2)
      assert k == round(k), (n, t, float(r))


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('fname', list(FILTERS))
def test_float32_copy_of_the_reference_sits_inside_the_bound(shape, fname):
  """The bound of the GPU test, checked on the host first: the reference evaluated in float32 (in the kernel's order, with its
  reduced translation) differs from the float64 one by no more than the bound, on every row of the GPU test; and the bound
  stays below 1e-4 max|S| (an indexing or alignment error is 0.1 max|S|)."""
  H, W = shape
  f = FILTERS[fname]
  S = R.image(1, 1, H, W, seed=H + W)[0, 0]
  for name, p in R.rows(H, W).items():
    ref = R.warp(S, p, f)
    got = R.warp(S, p, f, dtype=np.float32, reduce=True).astype(np.float64)
    if R.is_identity(p):
      assert np.array_equal(got, ref)
      continue
    bd = R.bound(S, p, f)
    assert bd.max() < 1e-4 * np.abs(S).max(), (name, bd.max())
    ratio = (np.abs(got - ref) / bd).max()
    assert ratio <= 1.0, (name, ratio)
  # ... and it is no loose bound: one sample of alignment error is thousands of times beyond it
  p = R.rows(H, W)['rot45']
  off = R.warp(np.roll(S, 1, axis=1), p, f)
  assert (np.abs(off - R.warp(S, p, f)) / R.bound(S, p, f)).max() > 100


# ---- the draws ----------------------------------------------------------------------------------------------------------
def test_draw_inverse_times_forward_is_identity(st):
  pipe = st.augment.AugmentPipe(0.8, seed=1)
  raw = pipe.sample(500)
  G = pipe.forward_maps(raw, 32, 48)
  inv = pipe.inverse_maps(G)
  assert np.abs(inv @ G - np.eye(3)).max() <= 1e-12
  params = pipe.params_of(raw, 32, 48)
  assert params.dtype == np.float32 and params.shape == (500, 8)
  assert np.array_equal(params[:, 2:6], inv[:, :2, :2].reshape(-1, 4).astype(np.float32))
  assert np.array_equal(params[:, 6:], inv[:, :2, 2].astype(np.float32))
  assert np.array_equal(params[:, 0], raw['xflip'].astype(np.float32))


def test_draw_composes_scale_rotation_anisotropy_translation(st):
  pipe = st.augment.AugmentPipe(1.0, seed=2)
  raw = pipe.sample(50)
  H, W = 16, 24
  G = pipe.forward_maps(raw, H, W)
  for b in range(50):
    s = 2.0 ** (0.2 * raw['scale'][b])
    w, phi, r = raw['rotate'][b], raw['aniso_phi'][b], 2.0 ** (0.2 * raw['aniso_r'][b])
    rot = lambda a: np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    lin = rot(phi) @ np.diag([r, 1 / r]) @ rot(-phi) @ rot(w) @ (s * np.eye(2))
    assert np.abs(G[b, :2, :2] - lin).max() <= 1e-12
    assert np.allclose(G[b, :2, 2], [0.125 * W * raw['translate'][b, 0], 0.125 * H * raw['translate'][b, 1]], rtol=0, atol=1e-12)


def test_labels_follow_the_table(st):
  pipe = st.augment.AugmentPipe(0.5, seed=3)
  raw = pipe.sample(400)
  L = pipe.labels_of(raw)
  fires = raw['fires']
  assert L.shape == (400, 9)
  assert set(np.unique(L[:, 0])) <= {0.0, 1.0} and set(np.unique(L[:, 1])) <= {0.0, 1.0}
  assert np.array_equal(L[:, 2], raw['scale'])
  assert np.allclose(L[:, 3], np.cos(raw['rotate']) - 1) and np.allclose(L[:, 4], np.sin(raw['rotate']))
  assert np.allclose(L[:, 5], raw['aniso_r'] * np.cos(raw['aniso_phi'])) and np.allclose(L[:, 6], raw['aniso_r'] * np.sin(raw['aniso_phi']))
  assert np.array_equal(L[:, 7:], raw['translate'])
  # a transform that does not fire draws 0 and labels 0
  cols = {0: [0], 1: [1], 2: [2], 3: [3, 4], 4: [5, 6], 5: [7, 8]}
  for t, cs in cols.items():
    assert not L[~fires[:, t]][:, cs].any(), st.augment.TRANSFORMS[t]
  assert np.abs(raw['rotate']).max() <= np.pi and np.abs(raw['aniso_phi']).max() <= np.pi
  # p = 0: every row is the identity and every label 0
  params, labels = st.augment.AugmentPipe(0.0).draw(16, 32, 32)
  assert all(R.is_identity(p) for p in params.numpy()) and not params[:, :2].any() and not labels.any()


def test_draws_are_seeded_and_leave_the_other_generators_alone(st):
  a, b = st.augment.AugmentPipe(0.5, seed=7), st.augment.AugmentPipe(0.5, seed=7)
  c = st.augment.AugmentPipe(0.5, seed=8)
  torch.manual_seed(11)
  before = torch.get_rng_state()
  pa, la = a.draw(32, 32, 32)
  assert torch.equal(torch.get_rng_state(), before), 'a draw consumed the default CPU generator'
  if torch.cuda.is_available():
    dev_before = torch.cuda.get_rng_state()
    a.draw(32, 32, 32), b.draw(32, 32, 32)
    assert torch.equal(torch.cuda.get_rng_state(), dev_before), 'a draw consumed the device generator'
    pa, la = a.draw(32, 32, 32)
  pb, lb = b.draw(32, 32, 32)
  pc, lc = c.draw(32, 32, 32)
  assert torch.equal(pa, pb) and torch.equal(la, lb)
  assert not torch.equal(pa, pc)
  assert pa.dtype == torch.float32 and la.dtype == torch.float32 and pa.device.type == 'cpu'


def test_every_transform_fires_at_rate_p(st):
  """20 000 samples at p = 0.12: each firing rate within 4 sigma of p (sigma = sqrt(p (1 - p) / n) = 0.0023)."""
  n, p = 20000, 0.12
  fires = st.augment.AugmentPipe(p, seed=0).sample(n)['fires']
  sigma = np.sqrt(p * (1 - p) / n)
  rates = fires.mean(axis=0)
  assert rates.shape == (6,)
  assert (np.abs(rates - p) <= 4 * sigma).all(), rates
  # and independently: the rate of any two together is p^2 within 4 sigma of that
  both = (fires[:, :, None] & fires[:, None, :]).mean(axis=0)[np.triu_indices(6, 1)]
  assert (np.abs(both - p * p) <= 4 * np.sqrt(p * p * (1 - p * p) / n)).all(), both


def test_default_filter(st):
  f = st.augment.default_filter()
  assert f.dtype == np.float32 and f.shape == (12,)
  assert np.array_equal(f, f[::-1]) and abs(float(f.astype(np.float64).sum()) - 1) <= 1e-7
  assert np.array_equal(f, R.default_filter())
  # each polyphase component sums to 1/2: a constant stays constant through the up pass
  assert abs(float(f[::2].astype(np.float64).sum()) - 0.5) <= 1e-7


# ---- every ValueError ----------------------------------------------------------------------------------------------------
def _edm_aug_config(st, **over):
  cfg = st.configs.edm_augment(tiny_config(st, 'vp'))
  for k, v in over.items():
    section, key = k.split('__')
    setattr(getattr(cfg, section), key, v)
  return cfg


def test_configs_edm_augment(st):
  base = st.configs.cifar10_ddpmpp_nll_st()
  cfg = st.configs.edm_augment(base)
  assert cfg.training.augment == 0.12 and cfg.model.augment_dim == 9 and cfg.training.sde == 'edm'
  plain = st.configs.edm(base)
  assert 'augment' not in plain.training and 'augment_dim' not in plain.model
  assert 'augment' not in base.training


def test_step_fn_value_errors_name_the_key(st):
  def make(cfg):
    return st.losses.get_step_fn(cfg, st.sde_lib.get_sde(cfg, None), train=True, optimize_fn=st.losses.optimization_manager(cfg))

  for bad in (-0.1, 1.5, float('nan'), 'x'):
    with pytest.raises(ValueError, match=r'config\.training\.augment'):
      make(_edm_aug_config(st, training__augment=bad))
  for bad in (0, 8, 10):
    with pytest.raises(ValueError, match=r'config\.model\.augment_dim'):
      make(_edm_aug_config(st, model__augment_dim=bad))
  for bad in (128, 6, 18 + 1):
    with pytest.raises(ValueError, match=r'config\.data\.image_size'):
      make(_edm_aug_config(st, data__image_size=bad))
  for bad in ([0.1, 0.4, 0.3, 0.2], [0.5, 0.25, 0.25], [1.0 / 14] * 14, [float('nan'), float('nan')]):
    with pytest.raises(ValueError, match=r'config\.training\.augment_filter'):
      make(_edm_aug_config(st, training__augment_filter=bad))
  # the feature is opt-in under every loss, and a symmetric filter of one's own is taken
  make(_edm_aug_config(st, training__augment_filter=[0.125, 0.375, 0.375, 0.125]))
  cfg = tiny_config(st, 'vp')
  cfg.training.augment, cfg.model.augment_dim = 0.3, 9
  make(cfg)
  ct = st.configs.consistency(tiny_config(st, 'vp'))
  ct.training.augment, ct.model.augment_dim = 0.3, 9
  make(ct)
  cfg0 = tiny_config(st, 'vp')
  cfg0.training.augment = 0                       # 0 is "absent": no augment_dim needed
  make(cfg0)


class _Stub(torch.nn.Module):
  """What get_step_fn needs of a score network with an augmentation embedding, without an engine: it records the batch and the
  labels in force at every evaluation."""

  def __init__(self):
    super().__init__()
    self.augment_dim = 9
    self._aug_ctx = None
    self.scale = torch.nn.Parameter(torch.ones(()))
    self.seen = []

  def forward(self, x, labels):
    self.seen.append((x.detach().clone(), None if self._aug_ctx is None else self._aug_ctx.clone()))
    return x * self.scale


@pytest.mark.parametrize('mixed', [False, True])
def test_labels_follow_the_micro_batches_and_the_mixed_halves(st, monkeypatch, mixed):
  """The host logic of the step with the launch left out (the pipe returns the images as they are, with the labels it drew):
  one pipe call per step on the whole batch, before the loss; every evaluated chunk sees the rows of the labels that belong to
  its images; the context is gone afterwards; the draws are those of a pipe seeded with config.seed."""
  calls = []

  def fake_call(self, images):
    params, labels = self.draw(*images.shape[:1], *images.shape[2:])
    calls.append(images.shape[0])
    return images, labels

  monkeypatch.setattr(st.augment.AugmentPipe, '__call__', fake_call)
  cfg = tiny_config(st, 'vp')
  cfg.training.augment, cfg.model.augment_dim, cfg.training.mixed, cfg.optim.num_micro_batch, cfg.seed = 1.0, 9, mixed, 2, 5
  sde = st.sde_lib.get_sde(cfg, None)
  model = _Stub()
  state = dict(optimizer=st.losses.get_optimizer(cfg, model.parameters()), model=model, step=0,
               ema=st.models.ema.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate))
  step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
  batch = st.datasets.synthetic_batch(cfg, 8, generator=torch.Generator().manual_seed(0))
  losses = step_fn(state, batch)
  _, want = st.augment.AugmentPipe(1.0, seed=5).draw(8, 16, 16)
  assert calls == [8] and model._aug_ctx is None and losses.shape == ((4,) if mixed else (8,))
  chunks = [(0, 2), (2, 4), (4, 6), (6, 8)] if mixed else [(0, 4), (4, 8)]
  assert len(model.seen) == len(chunks)
  for (x, labels), (lo, hi) in zip(model.seen, chunks):
    assert torch.equal(labels, want[lo:hi]) and x.shape[0] == hi - lo
  # a second step draws on: other labels
  model.seen.clear()
  step_fn(state, batch)
  assert not torch.equal(model.seen[0][1], want[:chunks[0][1]])


def test_pipe_value_errors(st):
  A = st.augment
  for bad in (-1, 2, None):
    with pytest.raises(ValueError):
      A.AugmentPipe(bad)
  with pytest.raises(ValueError, match='symmetric'):
    A.AugmentPipe(0.1, filter=[0.1, 0.2, 0.3, 0.4])
  pipe = A.AugmentPipe(0.1)
  for H, W in ((66, 64), (32, 33), (4, 4), (64, 128)):
    assert not A.shape_ok(H, W, 12)
    with pytest.raises(ValueError):
      pipe.check_shape(H, W)
  assert A.shape_ok(64, 64, 12) and A.shape_ok(8, 12, 2) and not A.shape_ok(32, 32, 14) and not A.shape_ok(32, 32, 3)


def test_augment_dim_needs_a_conditional_network(st):
  cfg = tiny_config(st, 'vp')
  cfg.model.augment_dim = 9
  cfg.model.conditional = False
  with pytest.raises(ValueError, match=r'config\.model\.augment_dim'):
    st.models.ncsnpp.NCSNpp(cfg, None)
  cfg.model.conditional = True
  cfg.model.augment_dim = -1
  with pytest.raises(ValueError, match=r'config\.model\.augment_dim'):
    st.models.ncsnpp.NCSNpp(cfg, None)


def _net(st, lib, augment_dim=None, num_classes=None):
  cfg = tiny_config(st, 'vp')
  if augment_dim is not None:
    cfg.model.augment_dim = augment_dim
  if num_classes is not None:
    cfg.model.num_classes = num_classes
  net = st.models.ncsnpp.NCSNpp(cfg, st.sde_lib.get_sde(cfg, None))
  net.set_backend(lib)
  return cfg, net


def test_augment_condition_checks_nests_and_restores(st, ref_lib):
  mu = st.models.utils
  _, net = _net(st, ref_lib, augment_dim=9)
  _, plain = _net(st, ref_lib)
  model = mu.DataParallel(net)
  with pytest.raises(ValueError, match=r'config\.model\.augment_dim'):
    with mu.augment_condition(plain, torch.zeros(2, 9)):
      pass
  for bad in (torch.zeros(2, 8), torch.zeros(9), torch.zeros(0, 9), torch.zeros(2, 9, dtype=torch.int64), [[0.0] * 9]):
    with pytest.raises(ValueError, match=r'config\.model\.augment_dim'):
      with mu.augment_condition(model, bad):
        pass
  assert net._aug_ctx is None and mu.augment_dim(model) == 9 and mu.augment_dim(plain) == 0
  a, b = torch.randn(3, 9), torch.randn(2, 9, dtype=torch.float64)
  with mu.augment_condition(model, a):
    assert torch.equal(net._aug_ctx, a) and torch.equal(net.augment_labels(3, a.device), a)
    with mu.augment_condition(net, b):
      assert net._aug_ctx.dtype == torch.float32 and torch.equal(net._aug_ctx, b.float())
    assert torch.equal(net._aug_ctx, a)
    with pytest.raises(ValueError, match='3 samples'):
      net.augment_labels(2, a.device)
  assert net._aug_ctx is None
  zeros = net.augment_labels(4, torch.device('cpu'))
  assert zeros.shape == (4, 9) and not zeros.any()
  assert plain.augment_labels(4, torch.device('cpu')) is None


def test_network_keys(st, ref_lib):
  cfg, plain = _net(st, ref_lib)
  _, zero = _net(st, ref_lib, augment_dim=0)
  _, aug = _net(st, ref_lib, augment_dim=9)
  _, both = _net(st, ref_lib, augment_dim=9, num_classes=3)
  sd0 = plain.state_dict()
  assert list(zero.state_dict()) == list(sd0) and not hasattr(plain, 'augment_emb')
  assert len(plain._flat_groups()) == len(zero._flat_groups()) == len(aug._flat_groups()) - 1
  assert list(aug.state_dict()) == list(sd0) + ['augment_emb.weight']
  assert list(both.state_dict()) == list(sd0) + ['class_emb.weight', 'augment_emb.weight']
  w = aug.state_dict()['augment_emb.weight']
  assert tuple(w.shape) == (4 * cfg.model.nf, 9) and not w.any() and aug.augment_emb.weight.requires_grad
  missing, unexpected = aug.load_state_dict(sd0, strict=False)
  assert missing == ['augment_emb.weight'] and not unexpected


def test_embedding_on_the_checker_is_refused_when_planned(st, ref_lib):
  _, net = _net(st, ref_lib, augment_dim=9)
  x, t = torch.randn(2, 3, 16, 16), torch.rand(2) * 999
  with pytest.raises(NotImplementedError, match='stk_augment.h'):
    net(x, t)
  _, plain = _net(st, ref_lib)
  assert plain(x, t).shape == x.shape
  from importlib import import_module
  _backend = import_module('soft-truncation_amd.op._backend')
  saved = _backend._backend
  _backend.set_backend(ref_lib)
  try:
    with pytest.raises(NotImplementedError, match='stk_augment.h'):
      st.augment.AugmentPipe(0.5)(torch.zeros(1, 1, 8, 8))
  finally:
    _backend.set_backend(saved)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_signature_table_covers_the_header(st):
  """include/stk_augment.h declares exactly the entries engine/lib.py binds, argument for argument; stk.h keeps its 84."""
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stk_augment.h')).read(), flags=re.S)
  decls = re.findall(r'\b(stk_[a-z0-9_]+)\s*\(([^)]*)\)', text)
  L = st.engine.lib
  table = L.SIGNATURES_AUGMENT
  assert sorted(n for n, _ in decls) == sorted(table) == ['stk_aug_embed_bwd_f32', 'stk_aug_embed_fwd_f32', 'stk_aug_ok',
                                                          'stk_aug_warp_f32']
  assert not set(table) & set(L.SIGNATURES) and len(L.SIGNATURES) == 84
  for name, args in decls:
    kinds = [L.P if '*' in a else {'int': L.I, 'long': L.L, 'float': L.F}[a.split()[0]] for a in args.split(',')]
    assert kinds == table[name], name
  row = [h for h in L.OPTIONAL_HEADERS if h.path == 'include/stk_augment.h']
  assert len(row) == 1 and row[0].has == 'has_augment' and row[0].table is table and row[0].restype == {}
  assert set(row[0].unchecked) == {'stk_aug_ok'}


def test_product_library_has_the_header_and_the_checker_has_not(st, ref_lib):
  lib = st.engine.lib.load()
  assert lib.has_augment is True and ref_lib.has_augment is False and not hasattr(ref_lib, 'aug_warp_f32')
  # the query needs no device; it is the rule the host checks restate
  for H, W, T in ((8, 8, 2), (64, 64, 12), (8, 12, 4), (66, 64, 12), (32, 31, 12), (32, 32, 14), (32, 32, 3), (6, 8, 2), (32, 32, 0)):
    assert bool(lib.aug_ok(H, W, T)) == st.augment.shape_ok(H, W, T), (H, W, T)


def test_package_exports(st):
  assert 'augment' in st.__all__ and st._REFERENCE_NAMES['augment'] is st.augment
