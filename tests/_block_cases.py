"""Stand-alone building-block cases shared by tests/test_gpu_blocks.py (HIP) and tests/test_blocks_cpu.py (the oracle's C
restatement as the backend): every module of the table in INTEGRATION.md "Building blocks on their own", against the
float64 restatement of tests/_block_ref.py -- the output, the gradient of every input and of every parameter."""
import torch
import torch.nn as nn

import _block_ref
from _util import close

# max|got - ref| / max|ref|: the split convolutions at their level (tests/_tolerances.py), blocks with a GroupNorm at the
# level tests/test_gpu_kernels.py::test_groupnorm holds the kernel to, attention at test_attention's
CONV_RTOL = 1e-5
GN_RTOL = 2e-5
ATTN_RTOL = 1e-4
FOURIER_RTOL = 2e-5


def _blocks(st):
  return {'L': st.models.layerspp, 'layers': st.models.layers, 'uds': st.models.up_or_down_sampling}


def construct(namespace, spec):
  """The module of a case's spec (module key, class name, args, kwargs) from `namespace` ({'L': layerspp, 'layers': ...,
  'uds': up_or_down_sampling}: this package's, or the reference's in tests/test_blocks_restatement.py)."""
  key, cls, a, kw = spec
  return getattr(namespace[key], cls)(*a, **kw)


def _biggan(**kw):
  return ('L', 'ResnetBlockBigGANpp', (), kw)


def _ddpm(**kw):
  return ('L', 'ResnetBlockDDPMpp', (), kw)


def _make(cls_path, *a, **kw):
  return (cls_path[0], cls_path[1], a, kw)


SILU = nn.SiLU
# id -> (builder, {input: shape}, rtol)
CASES = {
  'biggan_up_fir_temb_b3_16': (_biggan(act=SILU(), in_ch=64, out_ch=64, temb_dim=96, up=True, fir=True, dropout=0.),
                               {'x': (3, 64, 16, 16), 'temb': (3, 96)}, GN_RTOL),
  'biggan_down_naive_64to128_b1_32': (_biggan(act=SILU(), in_ch=64, out_ch=128, down=True, dropout=0., skip_rescale=False),
                                      {'x': (1, 64, 32, 32)}, GN_RTOL),
  'biggan_down_fir_temb_b3_32': (_biggan(act=SILU(), in_ch=128, out_ch=128, temb_dim=64, down=True, fir=True, dropout=0.),
                                 {'x': (3, 128, 32, 32), 'temb': (3, 64)}, GN_RTOL),
  'biggan_up_naive_128to64_b1_16': (_biggan(act=SILU(), in_ch=128, out_ch=64, temb_dim=64, up=True, dropout=0.),
                                    {'x': (1, 128, 16, 16), 'temb': (1, 64)}, GN_RTOL),
  'biggan_plain_temb_b3_16': (_biggan(act=SILU(), in_ch=128, out_ch=128, temb_dim=64, dropout=0.),
                              {'x': (3, 128, 16, 16), 'temb': (3, 64)}, GN_RTOL),
  'biggan_plain_norescale_b1_32': (_biggan(act=SILU(), in_ch=64, out_ch=64, dropout=0., skip_rescale=False),
                                   {'x': (1, 64, 32, 32)}, GN_RTOL),
  'biggan_elu_b3_16': (_biggan(act=nn.ELU(), in_ch=64, out_ch=128, temb_dim=32, dropout=0.),
                       {'x': (3, 64, 16, 16), 'temb': (3, 32)}, GN_RTOL),
  'biggan_relu_b1_16': (_biggan(act=nn.ReLU(), in_ch=64, out_ch=64, dropout=0.), {'x': (1, 64, 16, 16)}, GN_RTOL),
  'biggan_lrelu_b3_16': (_biggan(act=nn.LeakyReLU(0.2), in_ch=64, out_ch=64, temb_dim=32, dropout=0.),
                         {'x': (3, 64, 16, 16), 'temb': (3, 32)}, GN_RTOL),
  'ddpm_conv_shortcut_temb_b3_32': (_ddpm(act=SILU(), in_ch=64, out_ch=128, temb_dim=64, conv_shortcut=True, dropout=0.),
                                    {'x': (3, 64, 32, 32), 'temb': (3, 64)}, GN_RTOL),
  'ddpm_nin_shortcut_rescale_b1_16': (_ddpm(act=SILU(), in_ch=128, out_ch=64, dropout=0., skip_rescale=True),
                                      {'x': (1, 128, 16, 16)}, GN_RTOL),
  'ddpm_same_temb_b3_16': (_ddpm(act=SILU(), in_ch=64, temb_dim=64, dropout=0.),
                           {'x': (3, 64, 16, 16), 'temb': (3, 64)}, GN_RTOL),
  'attn_8_b3': (_make(('L', 'AttnBlockpp'), 128, skip_rescale=True), {'x': (3, 128, 8, 8)}, ATTN_RTOL),
  'attn_16_b1': (_make(('L', 'AttnBlockpp'), 64), {'x': (1, 64, 16, 16)}, ATTN_RTOL),
  'attn_32_b3': (_make(('L', 'AttnBlockpp'), 128, skip_rescale=True), {'x': (3, 128, 32, 32)}, ATTN_RTOL),
  'attn_32_b1': (_make(('L', 'AttnBlockpp'), 64), {'x': (1, 64, 32, 32)}, ATTN_RTOL),
  'combine_cat_b3_32': (_make(('L', 'Combine'), 3, 64, method='cat'), {'x': (3, 3, 32, 32), 'y': (3, 64, 32, 32)}, CONV_RTOL),
  'combine_sum_b1_16': (_make(('L', 'Combine'), 64, 128, method='sum'), {'x': (1, 64, 16, 16), 'y': (1, 128, 16, 16)},
                        CONV_RTOL),
  'conv2d_down_b3_32': (_make(('uds', 'Conv2d'), 64, 128, 3, down=True, kernel_init=lambda s: torch.randn(s) * 0.05),
                        {'x': (3, 64, 32, 32)}, CONV_RTOL),
  'conv2d_plain_b1_16': (_make(('uds', 'Conv2d'), 128, 64, 3, kernel_init=lambda s: torch.randn(s) * 0.05),
                         {'x': (1, 128, 16, 16)}, CONV_RTOL),
  'upsample_naive_conv_b3_16': (_make(('L', 'Upsample'), 64, with_conv=True), {'x': (3, 64, 16, 16)}, CONV_RTOL),
  'upsample_fir_b1_16': (_make(('L', 'Upsample'), 64, fir=True), {'x': (1, 64, 16, 16)}, CONV_RTOL),
  'downsample_naive_conv_b1_32': (_make(('L', 'Downsample'), 64, with_conv=True), {'x': (1, 64, 32, 32)}, CONV_RTOL),
  'downsample_fir_conv_b3_32': (_make(('L', 'Downsample'), 64, 128, with_conv=True, fir=True), {'x': (3, 64, 32, 32)},
                                CONV_RTOL),
  'downsample_naive_b3_16': (_make(('L', 'Downsample'), 64), {'x': (3, 64, 16, 16)}, CONV_RTOL),
  'nin_b3_16': (_make(('layers', 'NIN'), 64, 128), {'x': (3, 64, 16, 16)}, CONV_RTOL),
  'gaussian_fourier_b3': (_make(('L', 'GaussianFourierProjection'), 128, 1.0), {'x': (3,)}, FOURIER_RTOL),
  'fixed_fourier_rgb_b1_32': (_make(('L', 'FixedFouriereProjection')), {'x': (1, 3, 32, 32)}, FOURIER_RTOL),
  'fixed_fourier_gray_b3_16': (_make(('L', 'FixedFouriereProjection')), {'x': (3, 1, 16, 16)}, FOURIER_RTOL),
}


def build(st, case, device, backend=None, seed=0):
  """The module of `case` with random parameters (ones that init to zero would pin nothing), in eval mode, on `device`."""
  spec, shapes, rtol = CASES[case]
  torch.manual_seed(seed)
  m = construct(_blocks(st), spec)
  g = torch.Generator().manual_seed(seed + 1)
  with torch.no_grad():
    for n, p in m.named_parameters():
      if not p.requires_grad:
        continue
      if n.endswith('GroupNorm_0.weight') or n.endswith('GroupNorm_1.weight'):
        p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
      else:
        p.copy_(0.1 * torch.randn(p.shape, generator=g))
  m = m.to(device).eval()
  if backend is not None:
    m.set_backend(backend)
  return m, shapes, rtol


def inputs(case, device, seed=2, grad=True):
  _, shapes, _ = CASES[case]
  g = torch.Generator().manual_seed(seed)
  out = {}
  for n, s in shapes.items():
    t = torch.randn(s, generator=g)
    if case.startswith('fixed_fourier'):
      # sin / cos of 256 pi x: an fp32 argument carries |x| 256 pi 2^-24 of absolute error (the reference's too); on [0, 0.05]
      # that stays below the tolerance, the float64 yardstick has none
      t = 0.05 * torch.rand(s, generator=g)
    out[n] = t.to(device).requires_grad_(grad)
  return out


def check(st, case, device, backend=None, input_grads=True):
  """Forward, input and parameter gradients of one case against the float64 restatement."""
  m, _, rtol = build(st, case, device, backend)
  xs = inputs(case, device, grad=input_grads)
  out = m(**xs)
  gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(device)
  want_out, want_in, want_p = _block_ref.run(m, xs, gout)
  close(out, want_out, rtol=rtol, what=f'{case}: output')
  if not out.requires_grad:         # nothing to differentiate (a frozen projection of an input without gradient)
    assert not want_in and not want_p
    return m
  m.zero_grad(set_to_none=False)
  out.backward(gout)
  for n, t in xs.items():
    if t.requires_grad:
      close(t.grad, want_in[n], rtol=rtol, what=f'{case}: d{n}')
  named = dict(m.named_parameters())
  compare_param_grads({n: named[n].grad for n in want_p}, want_p, rtol, case)
  return m


def compare_param_grads(got, want, rtol, what, atol=1e-7):
  for n, w in want.items():
    # a bias gradient may vanish exactly (attention's key bias shifts every logit of a row alike): it is measured against
    # its layer's weight gradient as well
    pre, leaf = n.rsplit('.', 1) if '.' in n else ('', n)
    wname = (pre + '.' if pre else '') + {'b': 'W', 'bias': 'weight'}.get(leaf, leaf)
    floor = want[wname].abs().max().item() if wname != n and wname in want else 0.0
    close(got[n], w, rtol=rtol, atol=atol + rtol * floor, what=f'{what}: d{n}')
