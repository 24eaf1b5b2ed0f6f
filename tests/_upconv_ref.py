"""Float64 restatement of the FIR-upsampling convolution (include/stk_upconv.h; Conv2d(up=True), upsample_conv_2d), written
from its three formulas and nothing else -- in particular NOT as upsample_2d followed by a padded convolution, whose borders
differ.  The yardstick of tests/test_gpu_upconv.py; tests/test_upconv_cpu.py pins it to conv_transpose2d + upfirdn2d and to
autograd of itself.

  taps   kf = outer(k, k) / sum * gain * 4,  p = (len(k) - 2) - (K - 1),  pad = ((p + 1) // 2 + 1, p // 2 + 1)
  u      u[n,co,oy,ox] = sum_ci,kh,kw w[co,ci,kh,kw] z[n,ci,oy+kh-(K-1),ox+kw-(K-1)],  z[2i,2j] = x[i,j], zero elsewhere
  out    (upfirdn2d(u, kf, pad) + bias + res) / out_div
  dx     dx[n,ci,i,j]    = sum_co,kh,kw w[co,ci,kh,kw] du[n,co,2i+(K-1)-kh,2j+(K-1)-kw]
  dw     dw[co,ci,kh,kw] = sum_n,i,j    x[n,ci,i,j]    du[n,co,2i+(K-1)-kh,2j+(K-1)-kw]      du = adjoint of the FIR on dout

forward / grads derive the taps and the pad from a separable k as the model does; forward_taps / grads_taps take any KT x KT tap
array and any pad0, as the C ABI does (pad1 implied by the 2H x 2W output): tests/_upconv_cases.py runs on those, and
tests/test_upconv_cases_cpu.py pins them to the header's formulas.
"""
import torch
import torch.nn.functional as F


def taps_pad(k, K, gain=1.0, dtype=torch.float64):
  """(kf [KT, KT], (pad0, pad1)) of a 1-D or 2-D FIR kernel k (None: [1, 1]) for K x K weights."""
  k = torch.tensor([1, 1] if k is None else k, dtype=dtype)
  if k.dim() == 1:
    k = torch.outer(k, k)
  kf = k / k.sum() * (gain * 4)
  p = (kf.shape[0] - 2) - (K - 1)
  return kf, ((p + 1) // 2 + 1, p // 2 + 1)


def stuffed(x):
  """z: x with one zero between samples, (2H-1) x (2W-1)."""
  N, C, H, W = x.shape
  z = x.new_zeros(N, C, 2 * H - 1, 2 * W - 1)
  z[:, :, ::2, ::2] = x
  return z


def contraction(x, w):
  """u: z read as zero outside its range, so oy runs over 2H-2+K values."""
  K = w.shape[-1]
  return F.conv2d(F.pad(stuffed(x), [K - 1] * 4), w)      # conv2d is the correlation sum_kh,kw w[kh,kw] z[oy+kh, ox+kw]


def fir(u, kf, pad):
  """upfirdn2d(u, kf, pad) at 1:1: zero padding (a negative pad crops), then the true convolution with kf."""
  C = u.shape[1]
  up = F.pad(u, [pad[0], pad[1], pad[0], pad[1]])
  return F.conv2d(up, torch.flip(kf, [0, 1])[None, None].repeat(C, 1, 1, 1).to(u), groups=C)


def fir_adjoint(dout, kf, pad, UH, UW):
  """du[uy,ux] = sum_a,b kf[a,b] dout[uy + a - c, ux + b - c], c = KT - 1 - pad0, for uy < UH, ux < UW."""
  C, KT = dout.shape[1], kf.shape[0]
  c = KT - 1 - pad[0]
  OH, OW = dout.shape[2:]
  d = F.pad(dout, [c, UW + KT - 1 - c - OW, c, UH + KT - 1 - c - OH])
  return F.conv2d(d, kf[None, None].repeat(C, 1, 1, 1).to(dout), groups=C)


def pad_of(pad0, KT, K):
  """(pad0, pad1) of the C ABI's single pad0: the output is 2H x 2W, so pad1 = 2H - UH - pad0 + KT - 1 (include/stk_upconv.h)."""
  return pad0, KT + 1 - K - pad0


def forward_taps(x, w, kf, pad0, bias=None, res=None, out_div=1.0):
  """(out, u) for an arbitrary KT x KT tap array kf and an arbitrary pad0 (either pad may be negative: a crop)."""
  u = contraction(x, w)
  out = fir(u, kf, pad_of(pad0, kf.shape[0], w.shape[-1]))
  if bias is not None:
    out = out + bias.reshape(1, -1, 1, 1)
  if res is not None:
    out = out + res
  return out / out_div, u


def gather(x, w, du):
  """(dx, dw) of the two gather formulas from the map gradient du."""
  N, Cin, H, W = x.shape
  K = w.shape[-1]
  dx = torch.zeros_like(x)
  dw = torch.zeros_like(w)
  for kh in range(K):
    for kw in range(K):
      g = du[:, :, K - 1 - kh::2, K - 1 - kw::2][:, :, :H, :W]          # du[n, co, 2i+(K-1)-kh, 2j+(K-1)-kw]
      dx += torch.einsum('oc,noij->ncij', w[:, :, kh, kw], g)
      dw[:, :, kh, kw] = torch.einsum('ncij,noij->oc', x, g)
  return dx, dw


def grads_taps(x, w, dout, kf, pad0):
  """(dx, dw, du) for an arbitrary tap array and pad0."""
  H, W, K = x.shape[2], x.shape[3], w.shape[-1]
  du = fir_adjoint(dout, kf, pad_of(pad0, kf.shape[0], K), 2 * H - 2 + K, 2 * W - 2 + K)
  return gather(x, w, du) + (du,)


def forward(x, w, k=None, gain=1.0, bias=None, res=None, out_div=1.0):
  """(out, u) in the dtype of x."""
  kf, pad = taps_pad(k, w.shape[-1], gain, x.dtype)
  assert pad == pad_of(pad[0], kf.shape[0], w.shape[-1])
  return forward_taps(x, w, kf, pad[0], bias, res, out_div)


def grads(x, w, dout, k=None, gain=1.0):
  """(dx, dw, du) of out = fir(contraction(x, w)) for the output gradient dout, from the two gather formulas."""
  kf, pad = taps_pad(k, w.shape[-1], gain, x.dtype)
  return grads_taps(x, w, dout, kf, pad[0])
