"""Checks against the reference's own outputs: config values, checkpoint layout, initialisers and two less-travelled network
paths.  The reference's side of every case (tests/_ref_cases.py) was computed from the reference itself by
tools/make_golden.py (through oracle/refimport.py) and stored in tests/golden/ref_live.{json,npz}; this side runs here, on
any machine."""
import json
import os

import numpy as np
import pytest
import torch

import _ref_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def golden():
  with open(os.path.join(GOLDEN, 'ref_live.json')) as f:
    meta = json.load(f)
  return meta, dict(np.load(os.path.join(GOLDEN, 'ref_live.npz')))


@pytest.mark.parametrize('name', sorted(rc.FULL))
def test_config_values_match_reference(st, golden, name):
  """Every value of the restated BASELINE configs equals the reference's get_config()."""
  ref = golden[0]['configs'][name]
  ours = rc.flatten(st.configs.get_config(name))
  ours.pop('device')
  ours.pop('data.tfrecords_path', None)
  assert set(ref) == set(ours), (sorted(set(ref) - set(ours)), sorted(set(ours) - set(ref)))
  for k in ref:
    a, b = ref[k], ours[k]
    if isinstance(a, (tuple, list)):
      assert tuple(a) == tuple(b), k
    else:
      assert a == b, (k, a, b)


@pytest.mark.parametrize('name', sorted(rc.FULL))
def test_full_size_state_dict_matches_reference(st, golden, name):
  """Full-size models: parameter count, state_dict keys, order, shapes and dtypes (checkpoint compatibility)."""
  ref = golden[0]['full_size'][name]
  cfg = st.configs.get_config(name)
  cfg.device = torch.device('cpu')
  model = st.models.utils.DataParallel(st.models.ncsnpp.NCSNpp(cfg, None))
  ours = rc.layout(model)
  assert ours['n_params'] == rc.FULL[name][1] == ref['n_params']
  assert ours['state_dict'] == ref['state_dict']
  assert ours['requires_grad'] == ref['requires_grad']


def test_init_statistics_match_reference(st, golden):
  """Same initialisers: a fresh product model is bit-identical to the reference's (same fan computations, same RNG order)."""
  cfg = rc.init_config(st.configs.cifar10_ddpmpp_nll_st())
  torch.manual_seed(0)
  model = st.models.utils.DataParallel(st.models.ncsnpp.NCSNpp(cfg, None))
  want, got = golden[0]['init'], rc.digests(model.state_dict())
  assert list(got) == list(want)
  for k in want:
    assert got[k] == want[k], k     # same RNG consumption order and formulas -> identical tensors


def _seeded_state_dict(st, cfg, want_digests):
  """The product model under the case's seeds; its state_dict must be bit-identical to the one the reference's output came from."""
  torch.manual_seed(0)
  model = st.models.utils.DataParallel(st.models.ncsnpp.NCSNpp(cfg, None))
  rc.randomize_(model, torch.Generator().manual_seed(3))
  sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
  got = rc.digests(sd)
  assert list(got) == list(want_digests)
  for k in want_digests:
    assert got[k] == want_digests[k], k
  return sd


@pytest.mark.parametrize('name', rc.ACTIVATIONS)
def test_other_activations_match_reference(st, golden, name):
  """config.model.nonlinearity != 'swish' (models/layers.py:29-41; no shipped config uses it): the reference NCSNpp on a
  fixture-size config against the oracle RefNet on the same state_dict -- pins the oracle the product's activation codes are
  tested against (tests/test_engine_cpu.py::test_other_activations, tests/test_gpu_model.py::test_other_activations)."""
  import ref_torch
  meta, arrays = golden
  cfg = rc.activation_config(st.configs.cifar10_ddpmpp_nll_st(), name)
  ref = ref_torch.RefNet(cfg, _seeded_state_dict(st, cfg, meta['activations'][name]))
  x = torch.from_numpy(arrays[f'act_{name}_x'])
  t = torch.from_numpy(arrays[f'act_{name}_t'])
  want = torch.from_numpy(arrays[f'act_{name}_out'])
  ref.eval()
  with torch.no_grad():
    got = ref(x, t)
  err = float((got - want).abs().max() / want.abs().max())
  assert err <= 2e-6, (name, err)


def test_combine_cat_matches_reference(st, golden):
  """progressive_combine = 'cat' (Combine, models/layerspp.py:57-72; channel doubling models/ncsnpp.py:183-184) on the NCSN++
  pyramid config: the reference vs RefNet on the same state_dict, and the product module list has the reference's keys / shapes."""
  import ref_torch
  meta, arrays = golden
  cfg = rc.cat_config(st.configs.celebahq_uncsnpp_st())
  torch.manual_seed(0)
  model = st.models.utils.DataParallel(st.models.ncsnpp.NCSNpp(cfg, None))
  assert rc.layout(model)['state_dict'] == meta['cat_layout']['state_dict']
  ref = ref_torch.RefNet(cfg, _seeded_state_dict(st, cfg, meta['cat']))
  x, sig, want = (torch.from_numpy(arrays[k]) for k in ('cat_x', 'cat_sigma', 'cat_out'))
  ref.eval()
  with torch.no_grad():
    got = ref(x, sig)
  err = float((got - want).abs().max() / want.abs().max())
  assert err <= 2e-6, err
