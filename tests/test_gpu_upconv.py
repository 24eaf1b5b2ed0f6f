"""The FIR-upsampling convolution on the GPU (include/stk_upconv.h, csrc/upconv.hip): the three entries through ctypes, then the
modules that use them, against the float64 restatement of tests/_upconv_ref.py.  Every bound is max|got - ref| / max|ref| <=
CONV_RTOL (tests/_block_cases.py), the level the project holds its stride-2 f32-MFMA convolutions to.  The per-element bounds
on every launch form are tests/test_gpu_upconv_forms.py's.  (The taps of these cases, (1, 3, 3, 1) and (1, 1) normalised to sum
4, are dyadic: their float32 and float64 values are the same numbers, so the reference sees the taps the kernel receives.)

Worst measured error per direction over the kernel cases below (MI355X; profiles/upconv_accuracy.txt has every case):
  forward 8.762e-07, FIR adjoint (du) 2.029e-07, data gradient 2.441e-06, weight gradient 1.397e-06;
  three times the worst (7.323e-06) is inside the bound.
"""
import pytest
import torch

import _upconv_ref as ur
from _block_cases import CONV_RTOL
from _util import call

pytestmark = pytest.mark.gpu

F1331, F11 = (1, 3, 3, 1), (1, 1)
# id -> (N, Cin, Cout, H, W, K, k, bias, res, out_div)
CASES = {
  'b1_3to64_4x4_k3': (1, 3, 64, 4, 4, 3, F1331, True, True, 2.0 ** 0.5),
  'b3_64to3_8x8_k3_box': (3, 64, 3, 8, 8, 3, F11, False, False, 1.0),
  'b128_64to96_8x8_k3': (128, 64, 96, 8, 8, 3, F1331, True, True, 2.0 ** 0.5),
  'b128_256to96_8x8_k3': (128, 256, 96, 8, 8, 3, F1331, False, False, 1.0),
  'b3_96to256_16x16_k3': (3, 96, 256, 16, 16, 3, F1331, False, True, 1.0),
  'b1_256to64_32x32_k3': (1, 256, 64, 32, 32, 3, F1331, True, False, 2.0 ** 0.5),
  'b1_64to96_64x64_k3_box': (1, 64, 96, 64, 64, 3, F11, True, True, 1.0),
  'b3_96to64_6x12_k3': (3, 96, 64, 6, 12, 3, F1331, True, True, 2.0 ** 0.5),
  'b3_64to96_16x32_k1': (3, 64, 96, 16, 32, 1, F1331, True, True, 2.0 ** 0.5),
  'b1_256to256_8x8_k1_box': (1, 256, 256, 8, 8, 1, F11, False, False, 1.0),
  'b3_3to3_16x16_k3': (3, 3, 3, 16, 16, 3, F1331, True, False, 1.0),
  'b3_256to256_6x12_k3_box': (3, 256, 256, 6, 12, 3, F11, False, True, 2.0 ** 0.5),
}


def _rel(got, want):
  return (got.detach().cpu().double() - want).abs().max().item() / want.abs().max().item()


def _case(name, dev):
  N, Cin, Cout, H, W, K, k, bias, res, out_div = CASES[name]
  g = torch.Generator().manual_seed(sum(map(ord, name)))
  t = {'x': torch.randn(N, Cin, H, W, generator=g), 'w': torch.randn(Cout, Cin, K, K, generator=g) * 0.1,
       'bias': torch.randn(Cout, generator=g) if bias else None,
       'res': torch.randn(N, Cout, 2 * H, 2 * W, generator=g) if res else None,
       'dout': torch.randn(N, Cout, 2 * H, 2 * W, generator=g),
       'dx0': torch.randn(N, Cin, H, W, generator=g), 'dw0': torch.randn(Cout, Cin, K, K, generator=g)}
  kf, pad = ur.taps_pad(k, K, dtype=torch.float32)
  d = {n: (v.to(dev) if v is not None else None) for n, v in t.items()}
  d['fir'] = kf.contiguous().to(dev)
  dims = (N, H, W, Cin, Cout, K, kf.shape[0])
  return t, d, dims, pad[0], out_div, k


def _ws(lib, direction, dims, dev):
  nb = int(lib.upconv2d_ws_bytes(direction, *dims))
  assert nb >= 0
  # poisoned: a kernel that reads workspace nobody wrote fails loudly
  return torch.full((max(nb // 4, 64),), float('nan'), dtype=torch.float32, device=dev), nb


def _du(dims, dev):
  N, H, W, _, Cout, K, _ = dims
  return torch.full((N, Cout, 2 * H - 2 + K, 2 * W - 2 + K), float('nan'), dtype=torch.float32, device=dev)


def _f64(t):
  return None if t is None else t.double()


@pytest.mark.parametrize('name', sorted(CASES))
def test_forward(hip_lib, name):
  dev = torch.device('cuda:0')
  t, d, dims, pad0, out_div, k = _case(name, dev)
  N, H, W, _, Cout = dims[:5]
  y = torch.full((N, Cout, 2 * H, 2 * W), float('nan'), dtype=torch.float32, device=dev)
  ws, nb = _ws(hip_lib, 0, dims, dev)
  call(hip_lib, 'upconv2d_fwd_f32', d['x'], d['w'], d['fir'], d['bias'], d['res'], out_div, y, *dims, pad0, ws, nb)
  want, _ = ur.forward(_f64(t['x']), _f64(t['w']), k, bias=_f64(t['bias']), res=_f64(t['res']), out_div=out_div)
  err = _rel(y, want)
  print(f'upconv fwd {name}: rel err {err:.3e}')
  assert err <= CONV_RTOL, (name, err)


@pytest.mark.parametrize('name', sorted(CASES))
def test_dgrad_and_wgrad(hip_lib, name):
  """The data gradient fills du and overwrites (beta 0) or accumulates into (beta 0.5, alpha 0.75) dx; the weight gradient
  reads the du it left and accumulates alpha = 0.75 times its sums into a non-zero dw."""
  dev = torch.device('cuda:0')
  t, d, dims, pad0, _, k = _case(name, dev)
  dx_w, dw_w, du_w = ur.grads(_f64(t['x']), _f64(t['w']), _f64(t['dout']), k)
  du = _du(dims, dev)
  dx = torch.full_like(d['x'], float('nan'))
  call(hip_lib, 'upconv2d_dgrad_f32', d['dout'], d['w'], d['fir'], du, 0, dx, 0.0, 1.0, *dims, pad0)
  e_du, e_dx = _rel(du, du_w), _rel(dx, dx_w)
  dxa = d['dx0'].clone()
  call(hip_lib, 'upconv2d_dgrad_f32', None, d['w'], None, du, 1, dxa, 0.5, 0.75, *dims, pad0)
  e_dxa = _rel(dxa, 0.5 * _f64(t['dx0']) + 0.75 * dx_w)
  dw = d['dw0'].clone()
  ws, nb = _ws(hip_lib, 2, dims, dev)
  call(hip_lib, 'upconv2d_wgrad_f32', d['x'], None, None, du, 1, dw, 0.75, *dims, pad0, ws, nb)
  want_dw = _f64(t['dw0']) + 0.75 * dw_w
  e_dw = _rel(dw, want_dw)
  # the accumulated sums alone, against their own scale (dw0 must not hide an error of the sums)
  e_dws = ((dw.cpu().double() - _f64(t['dw0'])) / 0.75 - dw_w).abs().max().item() / dw_w.abs().max().item()
  print(f'upconv bwd {name}: du {e_du:.3e} dgrad {e_dx:.3e} dgrad(beta) {e_dxa:.3e} wgrad {e_dw:.3e} wgrad sums {e_dws:.3e}')
  assert e_du <= CONV_RTOL and e_dx <= CONV_RTOL and e_dxa <= CONV_RTOL and e_dw <= CONV_RTOL, (name, e_du, e_dx, e_dxa, e_dw)
  # dw0 ~ N(0, 1) carries half an ulp of its own into the difference: allow for it on top of the bound
  assert e_dws <= CONV_RTOL + 2.0 ** -23 * t['dw0'].abs().max().item() / 0.75 / dw_w.abs().max().item(), (name, e_dws)


@pytest.mark.parametrize('name', ['b128_64to96_8x8_k3', 'b1_256to64_32x32_k3', 'b3_64to96_16x32_k1', 'b3_3to3_16x16_k3'])
def test_wgrad_is_deterministic(hip_lib, name):
  """Two runs from dy (du_valid = 0), each into a fresh workspace and du: bit-identical."""
  dev = torch.device('cuda:0')
  t, d, dims, pad0, _, k = _case(name, dev)
  outs = []
  for _ in range(2):
    dw = d['dw0'].clone()
    ws, nb = _ws(hip_lib, 2, dims, dev)
    call(hip_lib, 'upconv2d_wgrad_f32', d['x'], d['dout'], d['fir'], _du(dims, dev), 0, dw, 1.25, *dims, pad0, ws, nb)
    outs.append(dw.cpu())
  assert torch.equal(outs[0], outs[1])
  _, dw_w, _ = ur.grads(_f64(t['x']), _f64(t['w']), _f64(t['dout']), k)
  err = _rel(outs[0], _f64(t['dw0']) + 1.25 * dw_w)
  print(f'upconv wgrad from dy {name}: rel err {err:.3e}')
  assert err <= CONV_RTOL, (name, err)


def test_bad_arguments_are_refused(hip_lib):
  dev = torch.device('cuda:0')
  _, d, dims, pad0, _, _ = _case('b1_3to64_4x4_k3', dev)
  ws, nb = _ws(hip_lib, 0, dims, dev)
  y = torch.empty(1, 64, 8, 8, device=dev)
  raw = hip_lib.upconv2d_fwd_f32.raw
  args = [d['x'].data_ptr(), d['w'].data_ptr(), d['fir'].data_ptr(), None, None, 1.0, y.data_ptr(), *dims, pad0, ws.data_ptr(), nb, 0]
  assert raw(*(args[:15] + [args[15], 16, 0])) == -1            # workspace too small
  assert raw(*(args[:5] + [0.0] + args[6:])) == -1               # out_div == 0
  bad = list(args)
  bad[12] = 5                                                    # K = 5
  assert raw(*bad) == -3


# ---- the modules ---------------------------------------------------------------------------------------------------------
def _module_ref(weight, bias, x, gout, k):
  x64 = x.detach().cpu().double().requires_grad_(True)
  w64 = weight.detach().cpu().double().requires_grad_(True)
  b64 = bias.detach().cpu().double().requires_grad_(True)
  out, _ = ur.forward(x64, w64, k, bias=b64)
  gx, gw, gb = torch.autograd.grad(out, [x64, w64, b64], gout.detach().cpu().double())
  # the gather formulas, not only autograd of the restatement's forward
  dx, dw, _ = ur.grads(x64.detach(), w64.detach(), gout.detach().cpu().double(), k)
  assert _rel(dx, gx) <= 1e-12 and _rel(dw, gw) <= 1e-12
  return out.detach(), dx, dw, gb


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('kind', ['conv2d_up', 'upsample_fir_conv', 'conv2d_up_1x1_box'])
def test_modules_match_float64(st, hip_lib, kind, batch):
  dev = torch.device('cuda:0')
  torch.manual_seed(3)
  if kind == 'conv2d_up':
    m, k, cin = st.models.up_or_down_sampling.Conv2d(64, 96, 3, up=True), F1331, 64
    conv = m
  elif kind == 'conv2d_up_1x1_box':
    m, k, cin = st.models.up_or_down_sampling.Conv2d(96, 64, 1, up=True, resample_kernel=F11), F11, 96
    conv = m
  else:
    m, k, cin = st.models.layerspp.Upsample(128, 64, with_conv=True, fir=True), F1331, 128
    conv = m.Conv2d_0
  g = torch.Generator().manual_seed(7)
  with torch.no_grad():
    for p in m.parameters():
      p.copy_(0.1 * torch.randn(p.shape, generator=g))
  m = m.to(dev).eval()
  x = torch.randn(batch, cin, 16, 16, generator=g).to(dev).requires_grad_(True)
  out = m(x)
  gout = torch.randn(out.shape, generator=g).to(dev)
  want, dx, dw, db = _module_ref(conv.weight, conv.bias, x, gout, k)
  m.zero_grad(set_to_none=False)
  out.backward(gout)
  errs = {'out': _rel(out, want), 'dx': _rel(x.grad, dx), 'dweight': _rel(conv.weight.grad, dw), 'dbias': _rel(conv.bias.grad, db)}
  print(f'upconv module {kind} b{batch}: ' + ' '.join(f'{n} {e:.3e}' for n, e in errs.items()))
  assert all(e <= CONV_RTOL for e in errs.values()), errs


@pytest.mark.parametrize('K,k', [(3, F1331), (1, F11), (3, None)])
def test_function_matches_float64(st, hip_lib, K, k):
  """upsample_conv_2d as a differentiable function (first order), gain included."""
  dev = torch.device('cuda:0')
  g = torch.Generator().manual_seed(11)
  x = torch.randn(3, 64, 8, 16, generator=g).to(dev).requires_grad_(True)
  w = (0.1 * torch.randn(96, 64, K, K, generator=g)).to(dev).requires_grad_(True)
  out = st.models.up_or_down_sampling.upsample_conv_2d(x, w, k=k, gain=1.5)
  gout = torch.randn(out.shape, generator=g).to(dev)
  gx, gw = torch.autograd.grad(out, [x, w], gout)
  x64, w64 = x.detach().cpu().double(), w.detach().cpu().double()
  want, _ = ur.forward(x64, w64, k, gain=1.5)
  dx, dw, _ = ur.grads(x64, w64, gout.cpu().double(), k, gain=1.5)
  errs = (_rel(out, want), _rel(gx, dx), _rel(gw, dw))
  print(f'upsample_conv_2d K{K} k{k}: out {errs[0]:.3e} dx {errs[1]:.3e} dw {errs[2]:.3e}')
  assert max(errs) <= CONV_RTOL, errs
