"""The tiny-network set-up the GPU tests of the add-on samplers share (test_gpu_dpm_solver.py, test_gpu_adaptive_sde.py)."""
import copy

from _model_cases import build_pair, tiny_config

_built = {}


def setup(st, lib, family, sampling):
  """(cfg, sde, model) of a tiny network in eval mode, `sampling` (a dict) assigned to cfg.sampling: built once per case."""
  key = (family, tuple(sampling.items()))
  if key not in _built:
    cfg = tiny_config(st, family)
    for k, v in sampling.items():
      setattr(cfg.sampling, k, v)
    cfg, _, sde, model, _ = build_pair(st, cfg, lib)
    model.eval()
    _built[key] = (cfg, sde, model)
  return _built[key]


def shape_of(cfg):
  return (2, cfg.data.num_channels, cfg.data.image_size, cfg.data.image_size)


def sampler(st, cfg, sde, eps, **options):
  """sampling.get_sampling_fn of a copy of cfg with `options` assigned to its cfg.sampling."""
  c = copy.deepcopy(cfg)
  for k, v in options.items():
    setattr(c.sampling, k, v)
  return st.sampling.get_sampling_fn(c, sde, shape_of(c), st.datasets.get_data_inverse_scaler(c), eps)
