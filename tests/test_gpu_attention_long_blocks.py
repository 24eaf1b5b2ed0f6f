"""AttnBlockpp above 16 x 16 on the streaming attention core (include/stk_attention_long.h): the stand-alone block
(engine/executor.ModuleExecutor) against the float64 restatement of tests/_block_ref.py, the plan of a 64 x 64 block
at batch 128, and a small NCSNpp with attention at 32 x 32 against the GEMM form of the same network."""
import importlib

import pytest
import torch

import _block_cases as cases
from _model_util import build_pair, patched_rng, rel_err

pytestmark = pytest.mark.gpu

cases.CASES.setdefault('attn_64_b2', (cases._make(('L', 'AttnBlockpp'), 128, skip_rescale=True), {'x': (2, 128, 64, 64)},
                                      cases.ATTN_RTOL))
MODEL_TOL = 2e-4      # tests/_model_cases.TOL


def _graph():
  return importlib.import_module('soft-truncation_amd.engine.graph')


def _attention_ops(programs):
  G = _graph()
  return [op for pr in programs.values() for op in pr.graph.ops if isinstance(op, G.AttentionCore)]


@pytest.mark.parametrize('case', ['attn_32_b3', 'attn_64_b2'])
def test_attnblockpp_on_streaming_core_matches_float64(st, hip_lib, case):
  """Output, input gradient and parameter gradients at 32 x 32 (B = 3) and 64 x 64 (B = 2), C = 128, at ATTN_RTOL."""
  m = cases.check(st, case, 'cuda')
  ops = _attention_ops(m.engine().programs)
  assert ops and all(op.long and not op.fused for op in ops)


def _plan_block(st, B, H):
  """The graph of a stand-alone AttnBlockpp (C = 128) on [B, 128, H, H], planned but not allocated or launched."""
  G = _graph()
  m, _, _ = cases.build(st, 'attn_64_b2', 'cuda')
  ex = m.engine()
  ex.ensure_flat()
  g = G.Graph(ex.flat, ex.lib)
  x = g.input('x', (B, 128, H, H), needs_grad=True)
  g.finalize(ex.emit(g, x=x), ex.lib)
  return g


def test_attnblockpp_64x64_batch128_plans_no_score_matrix(st, hip_lib, monkeypatch):
  """At 64 x 64 and B = 128 the block plans the streaming kernels: no [B, T, T] tensor, and an activation arena of
  seven [B, C, H, W] tensors (1.9 GB), 17 GB below the GEMM form's (whose score and probability matrices are 2 x 8.6 GB
  there)."""
  G = _graph()
  B, T = 128, 64 * 64
  g = _plan_block(st, B, 64)
  attn = [op for op in g.ops if isinstance(op, G.AttentionCore)]
  assert len(attn) == 1 and attn[0].long and not hasattr(attn[0], 's') and not hasattr(attn[0], 'p')
  assert not any(tuple(t.shape[-2:]) == (T, T) for t in g.tensors)
  act = 4 * g.act_size
  one = 4 * B * 128 * T                                     # bytes of one [B, C, H, W] activation: 0.27 GB
  assert act < 8 * one, act                                 # input, GroupNorm, q / k / v, o, output -- and nothing of T^2
  assert g.ws_bytes < 10 * one, g.ws_bytes                  # the planes of q, k, v, dO
  monkeypatch.setenv('STK_ATTN_FUSED', '0')
  gemm = _plan_block(st, B, 64)
  assert 4 * gemm.act_size - act >= 2 * 4 * B * T * T - 2 ** 24   # s and p, less the streaming form's lse / delta / rec
  print(f'AttnBlockpp 64x64 B=128: activation arena {act / 1e9:.2f} GB (GEMM form {4 * gemm.act_size / 1e9:.2f} GB), '
        f'workspace {g.ws_bytes / 1e9:.2f} GB')


def _net_config(st):
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st(), nf=32, ch_mult=(1, 2), image_size=32, attn_resolutions=(32, 16))
  cfg.sampling.method, cfg.sampling.predictor, cfg.sampling.corrector = 'pc', 'euler_maruyama', 'none'
  return cfg


def _net_run(st, lib):
  """Scores, input gradient and parameter gradients of one training-mode forward / backward, PC samples of one
  iteration, and the attention ops of the plans."""
  cfg, _, sde, model, _ = build_pair(st, _net_config(st), lib)
  dev = cfg.device
  g = torch.Generator().manual_seed(1)
  x = torch.randn(2, 3, 32, 32, generator=g)
  t = torch.rand(2, generator=g) * 0.9 + 0.05
  model.train()
  xg = x.clone().to(dev).requires_grad_(True)
  y = model(xg, (t * 999).to(dev))
  go = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(dev)
  (y * go).sum().backward()
  grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None}
  model.eval()
  sde.N = 1
  inv = st.datasets.get_data_inverse_scaler(cfg)
  fn = st.sampling.get_sampling_fn(cfg, sde, (2, 3, 32, 32), inv, 1e-3)
  with patched_rng(11):
    xs, _ = fn(model)
  ops = _attention_ops(model.module.engine().programs)
  return y.detach().cpu(), xg.grad.detach().cpu(), grads, xs.detach().cpu(), ops


def test_ncsnpp_with_attention_at_32x32_matches_gemm_form(st, hip_lib, monkeypatch):
  """attn_resolutions = (32, 16): the 32 x 32 blocks plan the streaming kernels, the 16 x 16 ones the short kernels;
  training-mode scores and gradients and one PC-sampler iteration agree with the GEMM form (STK_ATTN_FUSED=0) within
  the model tolerance."""
  y, gx, grads, xs, ops = _net_run(st, hip_lib)
  assert any(op.long and op.T == 1024 for op in ops) and any(op.fused and op.T == 256 for op in ops)
  assert not any(hasattr(op, 's') or hasattr(op, 'p') for op in ops)
  monkeypatch.setenv('STK_ATTN_FUSED', '0')
  y0, gx0, grads0, xs0, ops0 = _net_run(st, hip_lib)
  assert ops0 and not any(op.long or op.fused for op in ops0)
  assert rel_err(y, y0) <= MODEL_TOL, rel_err(y, y0)
  assert rel_err(gx, gx0) <= MODEL_TOL, rel_err(gx, gx0)
  scale = max(g.abs().max().item() for g in grads0.values())
  worst = max((grads[n] - grads0[n]).abs().max().item() for n in grads0) / scale
  assert worst <= MODEL_TOL, worst
  assert rel_err(xs, xs0) <= 5 * MODEL_TOL, rel_err(xs, xs0)
