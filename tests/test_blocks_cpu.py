"""The stand-alone building blocks on CPU, with the oracle's C restatement of include/stk.h injected as the backend (test-only,
as in tests/test_engine_cpu.py): the engine plumbing of engine/executor.ModuleExecutor -- programs, input and parameter
gradients, parameter placement -- against the float64 restatement of tests/_block_ref.py.  tests/test_gpu_blocks.py runs
the same cases on the HIP kernels."""
import pytest
import torch

import _block_cases as bc


@pytest.mark.parametrize('case', sorted(bc.CASES))
def test_block_matches_float64(st, ref_lib, case):
  # the checker does not implement include/stk_blocks.h: the Gaussian projection's input gradient is covered on the GPU only
  bc.check(st, case, 'cpu', ref_lib, input_grads=not case.startswith('gaussian'))


def test_gaussian_input_gradient_needs_the_blocks_header(st, ref_lib):
  m, _, _ = bc.build(st, 'gaussian_fourier_b3', 'cpu', ref_lib)
  with pytest.raises(NotImplementedError, match='stk_blocks.h'):
    m(torch.randn(3, requires_grad=True))


def test_block_of_a_bound_model_keeps_the_model_intact(st, ref_lib):
  import _model_util as mu
  cfg = mu.tiny_config(st, 'vp')
  model = mu.build_pair(st, cfg, ref_lib)[3]
  net = model.module
  x = torch.rand(2, 3, cfg.data.image_size, cfg.data.image_size)
  t = torch.rand(2) * 0.9 + 0.1
  with torch.no_grad():
    before = net(x, t)
  ptrs = [p.data_ptr() for p in net.parameters()]
  gptrs = [p.grad.data_ptr() for p in net.parameters() if p.requires_grad]
  flat, progs = net.engine().flat, dict(net.engine().programs)
  blk = next(m for m in net.modules() if isinstance(m, st.models.layerspp.ResnetBlockBigGANpp) or
             isinstance(m, st.models.layerspp.ResnetBlockDDPMpp))
  blk.set_backend(ref_lib)
  h = torch.randn(1, blk.in_ch, 8, 8, requires_grad=True)
  blk(h).sum().backward()
  assert blk.engine().flat is flat
  assert [p.data_ptr() for p in net.parameters()] == ptrs
  assert [p.grad.data_ptr() for p in net.parameters() if p.requires_grad] == gptrs
  with torch.no_grad():
    after = net(x, t)
  assert net.engine().flat is flat and net.engine().programs == progs
  assert torch.equal(before, after)


def test_free_block_moves_into_a_model_layout(st, ref_lib):
  """A free-standing block lays its parameters out on its own; a FlatParams made later over the same parameters (a model's
  re-layout) wins, and the block re-plans against it."""
  m, _, _ = bc.build(st, 'attn_8_b3', 'cpu', ref_lib)
  x = bc.inputs('attn_8_b3', 'cpu', grad=False)['x']
  y0 = m(x)
  own = m.engine().flat
  assert own.cols_block(m.qkv_params()[0]) is not None            # the q / k / v columns are interleaved
  other = st.engine.flat.FlatParams(list(m.parameters()), 'cpu', groups=m.engine()._own_groups())
  y1 = m(x)
  assert m.engine().flat is other and m.engine().flat is not own
  assert torch.equal(y0, y1)
