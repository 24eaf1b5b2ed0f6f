"""Host side of class conditioning (models/ncsnpp.py, models/utils.py class_condition, losses.get_step_fn): the ctypes table of
include/stk_cond.h, which library has it, the refusal of a conditional network on the checker, the state_dict keys with and
without classes, every ValueError of the context and of step_fn, nesting, and the label-dropout draw.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import _cond_ref as R
from _model_util import patched_rng, tiny_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(st, lib, family='vp', num_classes=None):
  cfg = tiny_config(st, family)
  if num_classes is not None:
    cfg.model.num_classes = num_classes
  net = st.models.ncsnpp.NCSNpp(cfg, st.sde_lib.get_sde(cfg, None))
  net.set_backend(lib)
  return cfg, net


def test_signature_table_covers_the_header(st):
  """include/stk_cond.h declares exactly the entries engine/lib.py binds, argument for argument; stk.h keeps its 84."""
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stk_cond.h')).read(), flags=re.S)
  decls = re.findall(r'\b(stk_[a-z0-9_]+)\s*\(([^)]*)\)', text)
  L = st.engine.lib
  table = L.SIGNATURES_COND
  assert sorted(n for n, _ in decls) == sorted(table) == ['stk_cfg_combine_f32', 'stk_class_embed_bwd_f32',
                                                          'stk_class_embed_fwd_f32']
  assert not set(table) & set(L.SIGNATURES) and len(L.SIGNATURES) == 84
  for name, args in decls:
    kinds = [L.P if '*' in a else {'int': L.I, 'long': L.L, 'float': L.F}[a.split()[0]] for a in args.split(',')]
    assert kinds == table[name], name
  row = [h for h in L.OPTIONAL_HEADERS if h.path == 'include/stk_cond.h']
  assert len(row) == 1 and row[0].has == 'has_cond' and row[0].table is table and row[0].restype == {}


def test_product_library_has_the_header_and_the_checker_has_not(st, ref_lib):
  assert st.engine.lib.load().has_cond is True
  assert ref_lib.has_cond is False
  assert not hasattr(ref_lib, 'cfg_combine_f32')


def test_conditional_network_on_the_checker_is_refused_when_planned(st, ref_lib):
  cfg, net = _net(st, ref_lib, num_classes=3)
  x, t = torch.randn(2, 3, 16, 16), torch.rand(2) * 999
  with pytest.raises(NotImplementedError, match='stk_cond.h'):
    net(x, t)
  # the unconditional network of the same config still runs there
  _, plain = _net(st, ref_lib)
  assert plain(x, t).shape == x.shape


@pytest.mark.parametrize('family', ['vp', 'rve'])
def test_unconditional_keys_are_unchanged(st, ref_lib, family):
  _, absent = _net(st, ref_lib, family)
  _, zero = _net(st, ref_lib, family, num_classes=0)
  keys = list(absent.state_dict())
  assert list(zero.state_dict()) == keys
  assert all(k == 'sigmas' or re.fullmatch(r'all_modules\.\d+\..+', k) for k in keys), keys
  assert not hasattr(absent, 'class_emb') and absent.num_classes == 0 and zero.num_classes == 0
  assert len(absent._flat_groups()) == len(zero._flat_groups())


@pytest.mark.parametrize('family', ['vp', 'rve'])
def test_conditional_adds_one_zero_table_behind_every_other_key(st, ref_lib, family):
  cfg, plain = _net(st, ref_lib, family)
  _, cond = _net(st, ref_lib, family, num_classes=3)
  sd, sd0 = cond.state_dict(), plain.state_dict()
  assert list(sd) == list(sd0) + ['class_emb.weight']
  assert all(sd[k].shape == sd0[k].shape for k in sd0)
  w = sd['class_emb.weight']
  dim = 4 * cfg.model.nf
  assert tuple(w.shape) == (4, dim) and not w.any()
  assert cond.class_emb.weight.requires_grad
  # an unconditional checkpoint is a warm start
  missing, unexpected = cond.load_state_dict(sd0, strict=False)
  assert missing == ['class_emb.weight'] and not unexpected


def test_num_classes_needs_a_conditional_network(st, ref_lib):
  cfg = tiny_config(st, 'vp')
  cfg.model.num_classes = 3
  cfg.model.conditional = False
  with pytest.raises(ValueError, match='conditional'):
    st.models.ncsnpp.NCSNpp(cfg, None)
  cfg.model.conditional = True
  cfg.model.num_classes = -1
  with pytest.raises(ValueError):
    st.models.ncsnpp.NCSNpp(cfg, None)


def test_context_checks_its_arguments(st, ref_lib):
  mu = st.models.utils
  _, net = _net(st, ref_lib, num_classes=3)
  model = mu.DataParallel(net)
  _, plain = _net(st, ref_lib)

  def enter(m, classes, guidance=0.0):
    with mu.class_condition(m, classes, guidance):
      pass

  with pytest.raises(ValueError, match='not class-conditional'):
    enter(plain, [0, 1])
  for bad in (torch.zeros(2, 2, dtype=torch.int64), torch.zeros((), dtype=torch.int64), torch.zeros(0, dtype=torch.int64), [], 3):
    with pytest.raises(ValueError):
      enter(model, bad)
  for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.bool), [0.0, 1.0], [True, False], ['a']):
    with pytest.raises(ValueError):
      enter(model, bad)
  for bad in ([0, 4], [-1, 0], torch.tensor([0, 4]), torch.tensor([-1])):
    with pytest.raises(ValueError, match=r'\[0, 3\]'):
      enter(model, bad)
  for bad in (float('nan'), float('inf'), -float('inf'), 'x', None):
    with pytest.raises(ValueError, match='guidance'):
      enter(model, [0, 1], bad)
  assert net._class_ctx is None
  enter(model, [0, 3, None, 2], 1.5)
  enter(net, torch.tensor([0, 3], dtype=torch.int32))


def test_contexts_nest_and_restore(st, ref_lib):
  mu = st.models.utils
  _, net = _net(st, ref_lib, num_classes=3)
  model = mu.DataParallel(net)
  assert net._class_ctx is None
  with mu.class_condition(model, [0, None, 2], guidance=1.5):
    cls, w, both = net._class_ctx
    assert cls.dtype == torch.float32 and cls.tolist() == [0.0, 3.0, 2.0] and w == 1.5
    assert both.tolist() == [0.0, 3.0, 2.0, 3.0, 3.0, 3.0]
    with mu.class_condition(net, torch.tensor([1, 1])):
      cls2, w2, both2 = net._class_ctx
      assert cls2.tolist() == [1.0, 1.0] and w2 == 0.0 and both2 is None
    assert net._class_ctx[0] is cls
    with pytest.raises(ValueError):          # a failed entry leaves the outer context in force
      with mu.class_condition(model, [7]):
        pass
    assert net._class_ctx[0] is cls
    with pytest.raises(RuntimeError, match='boom'):
      with mu.class_condition(model, [1]):
        raise RuntimeError('boom')
    assert net._class_ctx[0] is cls
  assert net._class_ctx is None


def test_a_batch_of_another_size_is_refused_at_evaluation(st, ref_lib):
  mu = st.models.utils
  _, net = _net(st, ref_lib, num_classes=3)
  with mu.class_condition(net, [0, 1, 2]):
    with pytest.raises(ValueError, match='3 classes'):
      net(torch.randn(2, 3, 16, 16), torch.rand(2) * 999)


class _Stub(torch.nn.Module):
  """What get_step_fn needs of a class-conditional score network, without an engine: it records the classes in force."""

  def __init__(self, num_classes):
    super().__init__()
    self.num_classes = num_classes
    self._class_ctx = None
    self.scale = torch.nn.Parameter(torch.ones(()))
    self.seen = []

  def forward(self, x, labels):
    self.seen.append(None if self._class_ctx is None else self._class_ctx[0].clone())
    return x * self.scale


def _step(st, num_classes, **training):
  cfg = tiny_config(st, 'vp')
  cfg.model.num_classes = num_classes
  for k, v in training.items():
    cfg.training[k] = v
  sde = st.sde_lib.get_sde(cfg, None)
  model = _Stub(num_classes)
  opt = st.losses.get_optimizer(cfg, model.parameters())
  ema = st.models.ema.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
  state = dict(optimizer=opt, model=model, ema=ema, step=0)
  step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
  return cfg, model, state, step_fn


def test_step_fn_value_errors(st):
  cfg, model, state, step_fn = _step(st, 3)
  batch = st.datasets.synthetic_batch(cfg, 4, generator=torch.Generator().manual_seed(0))
  with pytest.raises(ValueError, match='needs step_fn'):
    step_fn(state, batch)
  with pytest.raises(ValueError, match='3 classes'):
    step_fn(state, batch, [0, 1, 2])
  with pytest.raises(ValueError):
    step_fn(state, batch, [0, 1, 2, 4])
  cfg0, model0, state0, step_fn0 = _step(st, 0)
  with pytest.raises(ValueError, match='not class-conditional'):
    step_fn0(state0, batch, [0, 1, 2, 3])
  assert state['step'] == 0 and state0['step'] == 0 and not model.seen
  assert step_fn0(state0, batch).shape == (4,) and model0.seen == [None]


def test_label_dropout_draw_comes_first_and_reaches_the_model(st):
  cfg, model, state, step_fn = _step(st, 3, class_dropout=0.5)
  n = 8
  batch = st.datasets.synthetic_batch(cfg, n, generator=torch.Generator().manual_seed(0))
  classes = st.datasets.synthetic_classes(cfg, n, generator=torch.Generator().manual_seed(1))
  assert classes.dtype == torch.int64 and int(classes.min()) >= 0 and int(classes.max()) <= 2
  with patched_rng(9):
    first = torch.rand(n)                     # the first draw of the patched stream
  drop = first < 0.5
  assert drop.any() and not drop.all()
  with patched_rng(9):
    step_fn(state, batch, classes)
  assert len(model.seen) == 1 and model._class_ctx is None
  want = torch.where(drop, torch.tensor(3.0), classes.float())
  assert torch.equal(model.seen[0], want)
  # class_dropout = 0: nothing is drawn, the labels arrive as given and the loss sees the stream from its start
  cfg0, model0, state0, step_fn0 = _step(st, 3, class_dropout=0.0)
  np.random.seed(3)
  with patched_rng(9):
    l0 = step_fn0(state0, batch, classes)
  assert torch.equal(model0.seen[0], classes.float())
  cfgu, modelu, stateu, step_fnu = _step(st, 0)
  np.random.seed(3)
  with patched_rng(9):
    lu = step_fnu(stateu, batch)
  assert torch.equal(l0, lu)
  # the default is 0.1
  cfgd, modeld, stated, step_fnd = _step(st, 3)
  assert 'class_dropout' not in cfgd.training
  with patched_rng(9):
    step_fnd(stated, batch, classes)
  assert torch.equal(modeld.seen[0], torch.where(first < 0.1, torch.tensor(3.0), classes.float()))


def test_classes_follow_the_micro_batches_and_the_mixed_halves(st):
  cfg, model, state, step_fn = _step(st, 3, class_dropout=0.0, mixed=True)
  cfg.optim.num_micro_batch = 2
  step_fn = st.losses.get_step_fn(cfg, st.sde_lib.get_sde(cfg, None), train=True,
                                  optimize_fn=st.losses.optimization_manager(cfg))
  batch = st.datasets.synthetic_batch(cfg, 8, generator=torch.Generator().manual_seed(0))
  classes = torch.tensor([0, 1, 2, 3, 2, 1, 0, 3])
  losses = step_fn(state, batch, classes)
  assert losses.shape == (4,)
  assert [s.tolist() for s in model.seen] == [[0.0, 1.0], [2.0, 3.0], [2.0, 1.0], [0.0, 3.0]]


def test_restatement_decodes_indices_as_the_header_says():
  idx = torch.tensor([0.0, 2.0, 3.0, 4.0, -1.0, 1.5, float('nan'), float('inf')])
  assert R.class_row(idx, 3).tolist() == [0, 2, 3, 3, 3, 3, 3, 3]
  gy, g0 = torch.ones(3, 2), torch.zeros(3, 2)
  out, mag, count = R.embed_bwd_table(gy, torch.tensor([1.0, 1.0, 2.0]), g0)
  assert out.tolist() == [[0.0, 0.0], [2.0, 2.0], [1.0, 1.0]] and count.tolist() == [0, 2, 1]
