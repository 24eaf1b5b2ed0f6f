"""Host side of dynamic thresholding and guidance rescale (include/stk_guided.h, dpm_solver.py, models/utils.py) and the
yardsticks of their GPU tests: the ctypes table, the rank formula, the option plumbing and every ValueError, and the numpy
restatements of tests/_guided_ref.py against independent forms -- the selection against np.partition, the thresholded step
against a straight torch composition, the rescale against torch.std -- together with the conditions the GPU tests lean on
(nonzero sigma_g and |mean| <= 10 sigma on the rescale's inputs, an active threshold in the closed-form loop).  No GPU."""
import os
import re
import types
from importlib import import_module

import numpy as np
import pytest
import torch

import _dpm_ref as R
import _guided_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3


@pytest.fixture
def dpm(st):
  return st.dpm_solver


@pytest.fixture
def product_backend(st):
  """The `op` functions bound to the product library, whatever an earlier test bound them to."""
  backend = import_module('soft-truncation_amd.op._backend')
  saved = backend._backend
  backend.set_backend(st.engine.lib.load())
  yield backend
  backend.set_backend(saved)


# ---- the ABI table ------------------------------------------------------------------------------------------------------
def test_signature_table_covers_the_header(st):
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stk_guided.h')).read(), flags=re.S)
  decls = re.findall(r'\b(stk_[a-z0-9_]+)\s*\(([^)]*)\)', text)
  L = st.engine.lib
  table = L.SIGNATURES_GUIDED
  assert sorted(n for n, _ in decls) == sorted(table) == ['stk_abs_select_f32', 'stk_cfg_rescale_f32', 'stk_dpm_predict_f32',
                                                          'stk_dpm_threshold_update_f32', 'stk_guided_ws_bytes']
  assert not set(table) & set(L.SIGNATURES) and len(L.SIGNATURES) == 84
  kind = {'int': L.I, 'long': L.L, 'float': L.F}
  for name, args in decls:
    kinds = [L.P if '*' in a else kind[a.split()[0]] for a in args.split(',')]
    assert kinds == table[name], name
  row = [h for h in L.OPTIONAL_HEADERS if h.path == 'include/stk_guided.h']
  assert len(row) == 1 and row[0].has == 'has_guided' and row[0].table is table
  assert row[0].restype == {'stk_guided_ws_bytes': L.c_long} and tuple(row[0].unchecked) == ()
  assert L.OPTIONAL_HEADERS[-1] is row[0]


def test_product_library_has_the_header_and_the_checker_has_not(st, ref_lib):
  lib = st.engine.lib.load()
  assert lib.has_guided is True and ref_lib.has_guided is False and not hasattr(ref_lib, 'abs_select_f32')
  # the query answers without a device: 16 KiB of histograms per row, or the rescale's partial sums where they are larger
  assert int(lib.guided_ws_bytes(16, 3 * 256 * 256)) == 16 * 16384
  assert int(lib.guided_ws_bytes(3000, 4)) == 3000 * 16384
  assert int(lib.guided_ws_bytes(1, 3 * 256 * 256)) == 768 * 32
  assert int(lib.guided_ws_bytes(0, 4)) == -1 and int(lib.guided_ws_bytes(2, 2 ** 30)) == -3


# ---- host logic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p,n,want', [(0.995, 3072, 3056), (0.995, 315, 313), (1.0, 7, 6), (0.5, 1, 0), (1e-9, 5, 1)])
def test_rank_formula(dpm, p, n, want):
  assert dpm.threshold_rank(p, n) == want == G.rank_of(p, n)
  # the "higher" of the two order statistics the interpolated percentile lies between
  v = np.sort(np.random.RandomState(n).rand(n))
  assert v[max(want - 1, 0)] <= np.quantile(v, p) <= v[want]


def _config(st, **sampling):
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  cfg.sampling.method = 'dpm_solver'
  for k, v in sampling.items():
    setattr(cfg.sampling, k, v)
  return cfg


def test_threshold_options(st, dpm):
  cfg = _config(st)
  assert dpm.threshold_options(cfg) is None
  assert dpm.sampling_options(cfg) == (20, 2, 'logsnr', None)                 # still its four values
  assert dpm.threshold_options(_config(st, dpm_threshold=0.995)) == (0.995, 1.0)
  assert dpm.threshold_options(_config(st, dpm_threshold=0.9, dpm_threshold_floor=0.5)) == (0.9, 0.5)
  assert dpm.threshold_options(_config(st, dpm_threshold_floor=0.5)) is None, 'a floor alone switches nothing on'


def test_bad_arguments(st, dpm, product_backend):
  cfg = _config(st)
  sde = st.sde_lib.get_sde(cfg, None)
  build = lambda **kw: dpm.get_dpm_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v, steps=4, **kw)
  build(threshold=(0.995, 1.0))
  build(threshold=(1.0, 1e-3))
  with pytest.raises(ValueError, match='exclude each other'):
    build(threshold=(0.995, 1.0), clip=(-1., 1.))
  for p in (0.0, -0.5, 1.0001, float('nan')):
    with pytest.raises(ValueError, match='p must lie'):
      build(threshold=(p, 1.0))
  for floor in (0.0, -1.0, float('inf'), float('nan')):
    with pytest.raises(ValueError, match='floor must be'):
      build(threshold=(0.9, floor))
  with pytest.raises(ValueError, match=r'\(p, floor\)'):
    build(threshold=0.9)
  schedule = dpm.dpm_schedule(sde, 4, eps=EPS)
  with pytest.raises(ValueError, match='exclude each other'):
    dpm.dpm_sample(lambda x, t: x, torch.randn(1, 3, 4, 4), schedule, clip=(-1., 1.), threshold=(0.9, 1.0))
  with pytest.raises(ValueError, match='p must lie'):
    dpm.dynamic_threshold(torch.randn(1, 3, 4, 4), 1.5)
  # through the config keys
  with pytest.raises(ValueError, match='exclude each other'):
    st.sampling.get_sampling_fn(_config(st, dpm_threshold=0.9, dpm_clip=(-1., 1.)), sde, (2, 3, 8, 8), lambda v: v, EPS)
  with pytest.raises(ValueError, match='p must lie'):
    st.sampling.get_sampling_fn(_config(st, dpm_threshold=2.0), sde, (2, 3, 8, 8), lambda v: v, EPS)
  # thresholding is defined on centred data
  flat = _config(st, dpm_threshold=0.9)
  flat.data.centered = False
  with pytest.raises(ValueError, match='centred'):
    st.sampling.get_sampling_fn(flat, sde, (2, 3, 8, 8), lambda v: v, EPS)
  flat.sampling.dpm_threshold = None
  st.sampling.get_sampling_fn(flat, sde, (2, 3, 8, 8), lambda v: v, EPS)


def test_host_tensors_are_refused(st, dpm, product_backend):
  sde = st.sde_lib.VPSDE()
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    dpm.dpm_sample(lambda x, t: x, torch.randn(1, 3, 4, 4), dpm.dpm_schedule(sde, 4, eps=EPS), threshold=(0.9, 1.0))
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    dpm.dynamic_threshold(torch.randn(1, 3, 4, 4), 0.9)


def test_library_without_the_header_is_refused_when_the_sampler_is_built(st, dpm, product_backend):
  """A library that has stk_solver.h and not stk_guided.h: the plain sampler is built, the thresholded one is refused."""
  lib = st.engine.lib.load()
  old = types.SimpleNamespace(**{k: v for k, v in vars(lib).items() if k not in st.engine.lib.SIGNATURES_GUIDED})
  old.has_guided = False
  for name in st.engine.lib.SIGNATURES_GUIDED:
    if hasattr(old, name[4:]):
      delattr(old, name[4:])
  product_backend.set_backend(old)
  cfg = _config(st)
  sde = st.sde_lib.get_sde(cfg, None)
  dpm.get_dpm_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v)
  with pytest.raises(NotImplementedError, match='stk_guided.h'):
    dpm.get_dpm_sampler(cfg, sde, (2, 3, 8, 8), lambda v: v, threshold=(0.9, 1.0))
  with pytest.raises(NotImplementedError, match='stk_guided.h'):
    st.sampling.get_sampling_fn(_config(st, dpm_threshold=0.9), sde, (2, 3, 8, 8), lambda v: v, EPS)
  with pytest.raises(NotImplementedError, match='stk_guided.h'):
    dpm.dpm_sample(lambda x, t: x, torch.randn(1, 3, 4, 4), dpm.dpm_schedule(sde, 4, eps=EPS), threshold=(0.9, 1.0))
  with pytest.raises(NotImplementedError, match='stk_guided.h'):
    dpm.dynamic_threshold(torch.randn(1, 3, 4, 4), 0.9)


def _class_net(st, lib, num_classes=3):
  from _model_util import tiny_config
  cfg = tiny_config(st, 'vp')
  cfg.model.num_classes = num_classes
  torch.manual_seed(0)
  net = st.models.ncsnpp.NCSNpp(cfg, st.sde_lib.get_sde(cfg, None))
  net.set_backend(lib)
  return net


def test_class_condition_takes_and_restores_the_rescale(st, ref_lib):
  mu = st.models.utils
  net = _class_net(st, ref_lib)
  assert net._cfg_rescale == 0.0 and net._class_ctx is None
  for bad in (-0.1, 1.5, float('nan'), float('inf'), 'x', None):
    with pytest.raises(ValueError, match='rescale'):
      with mu.class_condition(net, [0, 1], 1.5, rescale=bad):
        pass
    assert net._cfg_rescale == 0.0 and net._class_ctx is None
  with mu.class_condition(net, [0, 1], 1.5, rescale=0.7):
    assert net._cfg_rescale == 0.7
    cls, w, both = net._class_ctx                                   # still the 3-tuple
    assert w == 1.5 and both.shape == (4,)
    with mu.class_condition(net, [2, 2], 2.0):
      assert net._cfg_rescale == 0.0 and net._class_ctx[1] == 2.0
      with mu.class_condition(net, [2, 2], rescale=1):
        assert net._cfg_rescale == 1.0 and net._class_ctx[1] == 0.0   # accepted with guidance 0: it does nothing
      assert net._cfg_rescale == 0.0
    with mu.classes_in_force(net, cls):
      assert net._cfg_rescale == 0.0
    assert net._cfg_rescale == 0.7 and net._class_ctx[1] == 1.5
  assert net._cfg_rescale == 0.0 and net._class_ctx is None
  with pytest.raises(RuntimeError, match='boom'):
    with mu.class_condition(net, [0, 1], 1.5, rescale=0.3):
      raise RuntimeError('boom')
  assert net._cfg_rescale == 0.0 and net._class_ctx is None


# ---- the restatements against independent forms ---------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,shifted', G.SHAPES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_select_restatement_is_np_partition(shape, shifted):
  B, n = shape
  for kind in G.CONTENTS:
    v = G.content(kind, B, n)
    assert v.dtype == np.float32 and v.shape == shape
    for rank in G.ranks(n):
      want = np.partition(np.abs(v), rank, axis=1)[:, rank]
      assert np.array_equal(G.bits(G.select(v, rank)), G.bits(want)), (kind, rank)
      # ... which is the order of the unsigned bit patterns of |v| (a NaN above +inf)
      keys = np.sort(G.bits(v) & np.uint32(0x7fffffff), axis=1)[:, rank]
      assert np.array_equal(keys, G.bits(want)), (kind, rank)


def test_contents_are_what_they_claim():
  B, n = 3, 315
  k = lambda kind: G.bits(np.abs(G.content(kind, B, n)))
  assert len(np.unique(k('equal'))) == 1
  assert len(np.unique(k('low-bits') >> 10)) == 1 and len(np.unique(k('low-bits'))) > 100
  assert len(np.unique(k('exponents') & 0x7fffff)) == 1 and len(np.unique(k('exponents') >> 23)) > 100
  v = G.content('straddle', B, n)
  for b in range(B):
    a = np.sort(np.abs(v[b]))
    mid = a[G.rank_of(0.5, n)]
    assert int((a == mid).sum()) == n // 2 and a[0] < mid < a[-1] and (v[b] == mid).any() and (v[b] == -mid).any()
  s = G.content('specials', 2, 12288)
  assert np.isinf(s).any() and (s == 0).any() and np.signbit(s[s == 0]).any() and (np.abs(s[s != 0]) < 1.2e-38).any()
  nan = G.content('one-nan', B, n)
  assert int(np.isnan(nan).sum()) == 1 and np.isnan(nan[0]).any()
  assert np.isnan(G.select(nan, n - 1)[0]) and not np.isnan(G.select(nan, n - 2)).any()


def test_thresholded_step_restatement_is_the_torch_composition():
  rng = np.random.RandomState(0)
  B, n = 3, 315
  x, s, p = (rng.standard_normal((B, n)) * sc for sc in (1.5, 2.0, 1.0))
  row = (1.3, 0.7, 0.45, 0.8, 0.35)
  for floor in (0.5, 2.5, 100.0):
    got_x, got_d, active = G.update(x, s, p, row, 0.9, floor)
    tx, ts, tp = (torch.from_numpy(v) for v in (x, s, p))
    d = row[0] * tx + row[1] * ts
    q = torch.quantile(d.abs(), 0.9, dim=1, interpolation='higher')
    sc = q.clamp_min(floor)[:, None]
    d = d.clamp(-sc, sc) / sc
    want_x = row[3] * tx + row[4] * (d + row[2] * (d - tp))
    assert np.allclose(got_d, d.numpy(), rtol=1e-14, atol=0) and np.allclose(got_x, want_x.numpy(), rtol=1e-13, atol=1e-15)
    assert np.array_equal(active, (q > floor).numpy())
    assert float(np.abs(got_d).max()) <= 1.0
    # step64, the form the kernel test uses, is the same step given the scale
    x64, d64, b_x, b_d = G.step64(x, s, p, row, sc[:, 0].numpy())
    assert np.array_equal(x64, got_x) and np.array_equal(d64, got_d)
    assert bool(np.all(np.abs(d64) <= b_d * (1 + 1e-15))) and bool(np.all(np.abs(x64) <= b_x * (1 + 1e-15)))
  assert active.sum() == 0, 'floor = 100 is never exceeded'
  # a NaN quantile poisons its row and no other
  s2 = s.copy()
  s2[1, 7] = np.nan
  _, d, _ = G.update(x, s2, None, row[:2] + (0.,) + row[3:], 1.0, 0.5)
  assert np.isnan(d[1]).all() and np.isfinite(d[[0, 2]]).all()
  # the fp32 restatement of the predict pass rounds three times
  x32, s32 = x.astype(np.float32), s.astype(np.float32)
  want = (torch.tensor(np.float32(1.3)) * torch.from_numpy(x32)) + (torch.tensor(np.float32(0.7)) * torch.from_numpy(s32))
  assert np.array_equal(G.bits(G.predict32(x32, s32, 1.3, 0.7)), G.bits(want.numpy()))


@pytest.mark.parametrize('shape,shifted', G.SHAPES[:1] + G.SHAPES[1:3] + G.SHAPES[4:],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_rescale_restatement_is_torch_std(shape, shifted):
  B, n = shape
  c, u = G.rescale_operands(B, n, constant_row=B - 1 if B > 1 else None)
  for w, phi in ((2.0, 0.7), (2.0, 1.0), (-0.5, 0.3), (7.5, 0.7)):
    w, phi = float(np.float32(w)), float(np.float32(phi))
    want, g, f = G.rescale64(c, u, w, phi)
    tc, tu = torch.from_numpy(c), torch.from_numpy(u)
    tg = tc + torch.tensor(np.float32(w)) * (tc - tu)
    assert np.array_equal(G.bits(g), G.bits(tg.numpy())), 'g is not the three fp32 roundings'
    sd_c, sd_g = tc.double().std(dim=1, unbiased=False), tg.double().std(dim=1, unbiased=False)
    live = sd_g > 0
    tf = torch.where(live, phi * sd_c / torch.where(live, sd_g, torch.ones_like(sd_g)) + (1 - phi), torch.ones_like(sd_g))
    assert np.allclose(f, tf.numpy(), rtol=1e-12, atol=0)
    assert np.allclose(want, (tf[:, None] * tg.double()).numpy(), rtol=1e-12, atol=0)
    # the conditions of the GPU test: every row but the constant one (and the single element) has sigma_g > 0 and
    # |mean| <= 10 sigma for c and for g, so sum(x x) / n - mean^2 in float64 loses nothing that 1 u of slack does not cover
    rows = slice(0, B - 1) if B > 1 else slice(0, 0)
    for a in (c.astype(np.float64)[rows], g.astype(np.float64)[rows]):
      assert bool(np.all(a.std(axis=1) > 0)) and bool(np.all(np.abs(a.mean(axis=1)) <= 10 * a.std(axis=1)))
    if B > 1:
      assert f[B - 1] == 1.0 and sd_g[B - 1] == 0
    else:
      assert f[0] == 1.0
  # phi = 0 and w = 0: the factor is exactly 1
  assert bool(np.all(G.rescale64(c, u, 2.0, 0.0)[2] == 1.0))
  want, g, f = G.rescale64(c, u, 0.0, 0.7)
  assert np.array_equal(G.bits(g), G.bits(c)) and bool(np.all(f.astype(np.float32) == 1.0))


@pytest.mark.parametrize('family', ['vp', 've'])
def test_closed_form_loop_keeps_the_threshold_active(family):
  """The loop the GPU test runs: thresholding is active on most (step, sample) pairs, the result is finite and inside
  [-1, 1] after the thresholded denoising evaluation, and fp32 arithmetic alone stays close to float64."""
  fam = R.VP(0.1, 20.) if family == 'vp' else R.VE(0.01, 50.)
  gauss = G.WideGaussian((4, 3, 8, 8))
  x_T = gauss.prior(*fam.alpha_sigma(1.0)).astype(np.float32)
  s = R.schedule(fam, 10, order=2, skip='logsnr', eps=EPS, T=1.)
  a, sg = s['alpha'], s['sigma']
  out = {}
  for dtype in (np.float64, np.float32):
    mu, c2 = gauss.mu.astype(dtype), (gauss.c ** 2).astype(dtype)
    score = lambda x, i: -(x - dtype(a[i]) * mu) / (dtype(a[i] ** 2) * c2 + dtype(sg[i] ** 2))
    out[dtype], active = G.sample(score, x_T, s, 0.9, 0.5, denoise=True, dtype=dtype)
    assert active > 0.5, f'{family}: thresholding active on {active:.2f} of the (step, sample) pairs'
  assert np.isfinite(out[np.float64]).all() and float(np.abs(out[np.float64]).max()) <= 1.0
  own = R.rel(out[np.float32], out[np.float64])
  print(f'{family}: thresholded loop, numpy fp32 deviates {own:.2e} from float64')
  assert 0 < own < 1e-4
