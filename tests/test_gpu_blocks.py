"""The NCSN++ building blocks called on their own, on the HIP kernels (engine/executor.ModuleExecutor): every module of the
table in INTEGRATION.md "Building blocks on their own" against the float64 restatement of tests/_block_ref.py (output, input
gradients, parameter gradients), and the engine's behaviour around them -- parameter placement inside a bound model,
parameter gradients only when autograd reaches them, program reuse, the device check, dropout seeding."""
import pytest
import torch

import _block_cases as bc
import _model_util as mu

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.mark.parametrize('case', sorted(bc.CASES))
def test_block_matches_float64(st, hip_lib, case):
  bc.check(st, case, DEV, hip_lib)


def _first_resblock(st, net):
  L = st.models.layerspp
  return next(m for m in net.modules() if isinstance(m, (L.ResnetBlockBigGANpp, L.ResnetBlockDDPMpp)))


def test_block_of_a_bound_model_keeps_the_model_intact(st, hip_lib):
  cfg = mu.tiny_config(st, 'vp')
  net = mu.build_pair(st, cfg, hip_lib)[3].module
  S = cfg.data.image_size
  x = torch.rand(2, 3, S, S, generator=torch.Generator().manual_seed(1)).to(DEV)
  t = (torch.rand(2, generator=torch.Generator().manual_seed(2)) * 0.9 + 0.1).to(DEV)
  net.eval()
  with torch.no_grad():
    before = net(x, t)
  ex = net.engine()
  flat, progs = ex.flat, dict(ex.programs)
  ptrs = [p.data_ptr() for p in net.parameters()]
  gptrs = [p.grad.data_ptr() for p in net.parameters() if p.requires_grad]
  blk = _first_resblock(st, net)
  h = torch.randn(3, blk.in_ch, 16, 16, device=DEV, requires_grad=True)
  blk(h).square().sum().backward()
  assert blk.engine().flat is flat                       # planned against the model's own buffers
  assert [p.data_ptr() for p in net.parameters()] == ptrs
  assert [p.grad.data_ptr() for p in net.parameters() if p.requires_grad] == gptrs
  with torch.no_grad():
    after = net(x, t)
  assert ex.flat is flat and ex.programs == progs
  assert torch.equal(before, after)


def test_param_grads_only_when_autograd_reaches_them(st, hip_lib):
  m, _, _ = bc.build(st, 'biggan_plain_temb_b3_16', DEV, hip_lib)
  xs = bc.inputs('biggan_plain_temb_b3_16', DEV)
  m(**xs).sum().backward()
  snap = {n: p.grad.clone() for n, p in m.named_parameters()}
  gx, = torch.autograd.grad(m(**xs).sum(), xs['x'])
  assert gx.abs().max() > 0
  for n, p in m.named_parameters():
    assert torch.equal(p.grad, snap[n]), n
  m(**xs).sum().backward()
  for n, p in m.named_parameters():
    assert torch.allclose(p.grad, 2 * snap[n], rtol=1e-5, atol=1e-6), n


def test_second_backward_of_one_forward_raises(st, hip_lib):
  m, _, _ = bc.build(st, 'nin_b3_16', DEV, hip_lib)
  out = m(**bc.inputs('nin_b3_16', DEV))
  out.sum().backward(retain_graph=True)
  with pytest.raises(RuntimeError, match='backward called twice'):
    out.sum().backward()


def test_equal_shapes_reuse_the_program(st, hip_lib):
  m, _, _ = bc.build(st, 'attn_16_b1', DEV, hip_lib)
  x = bc.inputs('attn_16_b1', DEV)['x']
  first = m(x)
  ex = m.engine()
  progs = dict(ex.programs)
  for _ in range(3):
    again = m(x)
    again.sum().backward()
  assert ex.programs == progs
  assert torch.equal(first, m(x))
  if ex._graphs_on():
    assert ex.graph_replays > 0                           # the repeated calls replay the captured forward


def test_cpu_input_raises(st, hip_lib):
  m, _, _ = bc.build(st, 'nin_b3_16', DEV, hip_lib)
  with pytest.raises(RuntimeError, match='HIP kernels only'):
    m(torch.randn(3, 64, 16, 16))
  cpu_block = st.models.layers.NIN(64, 64)
  with pytest.raises(RuntimeError, match='HIP kernels only'):
    cpu_block(torch.randn(1, 64, 8, 8))


def test_training_dropout_follows_the_seed(st, hip_lib):
  L = st.models.layerspp
  torch.manual_seed(0)
  m = L.ResnetBlockBigGANpp(torch.nn.SiLU(), 64, 64, temb_dim=32, dropout=0.3).to(DEV).train()
  x = torch.randn(3, 64, 16, 16, device=DEV)
  t = torch.randn(3, 32, device=DEV)
  outs = []
  for seed in (7, 7, 8):
    torch.manual_seed(seed)
    outs.append(m(x, t))
  assert torch.equal(outs[0], outs[1])
  assert not torch.equal(outs[0], outs[2])
  m.eval()
  assert torch.equal(m(x, t), m(x, t))
