"""The float64 restatement of the building blocks (tests/_block_ref.py), the yardstick of tests/test_gpu_blocks.py, against the
reference's own blocks built with the same parameters: float64 on both sides, so only the order of operations differs.
Needs the reference's sources on this machine (oracle/refimport.py); skipped where they are absent."""
import pytest
import torch

import _block_cases as bc
import _block_ref
from _util import close

RTOL = 1e-10


@pytest.fixture(scope='module')
def ref_blocks():
  import refimport
  if not refimport.available():
    pytest.skip('the reference is not present on this machine')
  ns = refimport.load()
  return {'L': ns.layerspp, 'layers': ns.layers, 'uds': ns.uds}


def _reference_forward(ref, ref_blocks, ins):
  try:
    return ref(**ins)
  except ValueError as e:
    # Upsample(fir=False) calls F.interpolate(x, (2H, 2W), 'nearest'): the third positional parameter is scale_factor, and
    # current torch refuses size and scale_factor together.  Its intent -- nearest-neighbour x2, then Conv_0 -- is the
    # reference's own naive_upsample_2d followed by Conv_0.
    if type(ref).__name__ != 'Upsample' or ref.fir or 'scale_factor' not in str(e):
      raise
    h = ref_blocks['uds'].naive_upsample_2d(ins['x'], factor=2)
    return ref.Conv_0(h) if ref.with_conv else h


@pytest.mark.parametrize('case', sorted(bc.CASES))
def test_restatement_matches_reference(st, ref_blocks, case, monkeypatch):
  ours, _, _ = bc.build(st, case, 'cpu')
  spec = bc.CASES[case][0]
  torch.manual_seed(0)
  ref = bc.construct(ref_blocks, spec)
  ref.load_state_dict(ours.state_dict())
  ref = ref.double().eval()
  # the reference's FIR helpers build their taps as fp32 tensors (exact for the (1, 3, 3, 1) kernels); its CPU upfirdn2d then
  # wants them in the input's dtype
  fir = ref_blocks['uds'].upfirdn2d
  monkeypatch.setattr(ref_blocks['uds'], 'upfirdn2d', lambda x, k, *a, **kw: fir(x, k.to(x.dtype), *a, **kw))
  xs = bc.inputs(case, 'cpu')
  ins = {n: t.detach().double().requires_grad_() for n, t in xs.items()}
  out = _reference_forward(ref, ref_blocks, ins)
  gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
  want_out, want_in, want_p = _block_ref.run(ours, xs, gout)
  close(out, want_out, rtol=RTOL, atol=0.0, what=f'{case}: output')
  params = {n: p for n, p in ref.named_parameters() if p.requires_grad}
  grads = torch.autograd.grad(out, list(ins.values()) + list(params.values()), gout)
  for (n, _), g in zip(ins.items(), grads):
    close(g, want_in[n], rtol=RTOL, atol=0.0, what=f'{case}: d{n}')
  bc.compare_param_grads(dict(zip(params, grads[len(ins):])), want_p, RTOL, case, atol=1e-15)
