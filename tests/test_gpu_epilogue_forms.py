"""The straight-line epilogues of the split GEMMs (EpFwd, EpDgrad, EpSlab, EpWgrad of csrc/conv.hip), branch by branch.

Every output, gradient and scratch buffer lies between sentinel guards (tests/_stream_util.py Guarded) and is pre-filled
with a sentinel value; after the call the guards are intact, every element the call must not write still holds the
sentinel, and every written element EQUALS the exact-operand three-term model of tests/_conv_split_ref.py bit for bit
(operands h + l, dyadic bias / temb / res / old gradients, out_div in {1, 2}, alpha and beta in {1, 0.5, 0}: all sums are
exact in fp32 in any order, so there is no tolerance).  Every case asserts through the library's own diagnostics that it
reaches the kernel it was written for.

Shapes.  Map size, channel counts, dead rows, images per tile and the routing of rows are the ones the epilogues' branches
depend on, at their smallest.  The batch is NOT the smallest: the plan (split_plan of csrc/conv.hip) hands a launch to the
un-split kernels only from 192 output tiles on, and to the split path only for M >= 96 rows and first sources of a
multiple of 32 channels, so
  - the 16 x 16 halo forward (Cin 32, Cout 96: rows 96 .. 127 of the tile dead) runs at N = 96 (192 tiles), not 2;
  - the un-split 8 x 8 forward (Cout 160) at N = 191: 12224 pixels, the last tile half dead, as with N = 3;
  - temb across images: 4 x 4 maps at N = 1536 (8 images per tile, staged), 2 x 2 maps at N = 6144 (32 images: unstaged);
  - the two-source 1 x 1 forward of the f32-operand entry: C1 = 64 (a multiple of 32), C2 = 32, Cout = 160 (>= 96), 51 maps
    of 12 x 20 (12240 pixels: a ragged last tile);
  - the 1 x 1 weight gradient: Cin = 80 (the plan wants >= 64; 48 dead columns in the tile), Cout = 160.
With the smaller figures the same calls run on the f32-operand MFMA kernels, whose full products (lo lo included) no exact
model describes.  With the plain-C checker standing in (STK_SELFCHECK, no GPU) the results are compared with the model
plus its lo lo term, under a tolerance: that mode checks this file, not the kernels."""
import functools

import numpy as np
import pytest
import torch

import _conv_split_ref as cr
from _conv_split_cases import _bytes
from _stream_util import Guarded
from _util import call, dev_of

pytestmark = pytest.mark.gpu

SENT = np.float32(-24680.5)           # no exact result comes near it


def _dyadic(shape, top, seed):
  return (np.random.default_rng(seed).integers(-4 * top, 4 * top + 1, shape) / 4.0).astype(np.float32)


def _sent(shape):
  return np.full(shape, SENT, np.float32)


@functools.lru_cache(maxsize=2)
def _operands(N, Kc, M, H, W, K, layout, dgrad):
  """exact activation operand a [N, Kc, H, W], the weight tensor of the layer, its GEMM view, and the contraction"""
  hmax = 2 if Kc * K * K <= 864 else 1
  a = cr.exact_tensor((N, Kc, H, W), hmax, 1)
  Cin, Cout = (M, Kc) if dgrad else (Kc, M)
  w = cr.exact_tensor((Cin, Cout) if layout == 1 else (Cout, Cin, K, K), hmax, 2)
  Wg = cr.gemm_weights(w, layout, Cin, Cout, K, dgrad)
  acc = cr.three_term_acc(cr.problem(dgrad, a, Wg, K * K))
  return a, w, Wg, acc


def _equal(got, want, lolo, lib, what):
  if not lib.is_device:               # the checker multiplies in full
    assert np.allclose(got, want + lolo, rtol=0, atol=1e-3), what
    return
  off = got.astype(np.float64) != want
  if off.any():
    i = np.unravel_index(int(np.abs(got - want).argmax()), got.shape)
    raise AssertionError(f'{what}: {int(off.sum())} of {off.size} elements differ from the three-term model; the farthest at '
                         f'{tuple(int(j) for j in i)}: got {float(got[i])!r}, want {float(want[i])!r}')


def _planes_of(lib, g_a, a, d):
  N, Kc, H, W = a.shape
  rec = torch.zeros(256, device=d)
  call(lib, 'amax_partial_f32', g_a.view, a.size, rec)
  planes = torch.zeros(int(lib.planes_bytes(N, Kc, H * W)), dtype=torch.uint8, device=d)
  call(lib, 'split_planes_f32', g_a.view, N, Kc, H * W, rec, 256, planes)
  return planes, rec


def _assert_form(lib, di, dims, K, form):
  """form: 'h16' (halo GEMM), 'g' (un-split x2d::gemm_kernel) or 'ks' (EpSlab + slab sum); device only"""
  C1, C2, N, H, W, Cout = dims
  assert int(lib.conv2d_pl_ok(di, C1, C2, N, H, W, Cout, K, K, 1, K // 2)) == 1, dims
  if not lib.is_device:
    return
  ks = int(lib.conv2d_pl_ksplit(di, C1, C2, N, H, W, Cout, K, K))
  halo = int(lib.conv2d_pl_halo(di, C1, C2, N, H, W, Cout, K, K))
  got = 'ks' if ks > 1 else (f'h{halo}' if halo else 'g')
  assert got == form, (dims, got, ks, halo)


def _forward(lib, N, Cin, Cout, H, W, K, form, opts, entry='pl', S1=0, splits=None):
  """one forward call; opts: subset of {'bias', 'temb', 'res', 'div'}"""
  d = dev_of(lib)
  a, w, Wg, acc = _operands(N, Cin, Cout, H, W, K, 0, False)
  bias = _dyadic((Cout,), 2, 3) if 'bias' in opts else None
  temb = _dyadic((N, Cout + 8), 2, 4) if 'temb' in opts else None          # read as the column slice [0, Cout) of a wider tensor
  res = _dyadic((N, Cout, H, W), 4, 5) if 'res' in opts else None
  div = 2.0 if 'div' in opts else 1.0
  C1, C2 = (S1, Cin - S1) if S1 else (Cin, 0)
  dims = (C1, C2, N, H, W, Cout)
  if entry == 'pl':
    _assert_form(lib, 0, dims, K, form)
  elif lib.is_device:
    assert int(lib.conv2d_variant(0, C1, C2, N, H, W, Cout, H, W, K, K, 1, K // 2, 0)) == 5, dims
  nb = int(lib.conv2d_fwd_ws_bytes(C1, C2, N, H, W, Cout, K, K, 1, K // 2))
  assert nb > 0 or not lib.is_device
  srcs = [np.ascontiguousarray(a[:, :C1]), np.ascontiguousarray(a[:, C1:])] if C2 else [a]
  g_src = [Guarded(s, d) for s in srcs]
  g_w = Guarded(w, d)
  g_in = {k: Guarded(v, d) for k, v in (('bias', bias), ('temb', temb), ('res', res)) if v is not None}
  g_y, g_ws = Guarded(_sent((N, Cout, H, W)), d), Guarded(_bytes(nb), d)
  ep = (g_w.view, 0, g_in['bias'].view if bias is not None else None, g_in['temb'].view if temb is not None else None,
        Cout + 8 if temb is not None else 0, g_in['res'].view if res is not None else None, div, g_y.view, N, H, W, Cout)
  if entry == 'pl':
    planes, rec = _planes_of(lib, g_src[0], a, d)
    call(lib, 'conv2d_fwd_pl_f32', planes, rec, Cin, *ep, K, K, None, g_ws.view, nb)
  else:
    call(lib, 'conv2d_fwd_f32', g_src[0].view, C1, g_src[1].view if C2 else None, C2, *ep, H, W, K, K, 1, K // 2,
         g_ws.view, nb)
  if lib.is_device:
    torch.cuda.synchronize()
  what = f'fwd {dims} {K}x{K} {sorted(opts)}'
  for g in [g_y, g_ws, g_w] + g_src + list(g_in.values()):
    g.check(what)
  p = cr.problem(False, a, Wg, K * K, splits, bias, None if temb is None else np.ascontiguousarray(temb[:, :Cout]), res, div)
  t = cr.three_term(p, acc=acc)
  got = g_y.view.cpu().numpy()
  assert not (got == SENT).any(), f'{what}: {int((got == SENT).sum())} output elements were not written'
  _equal(got, t['out'], t['lolo'], lib, what)


OPTS = [frozenset(o for o, on in zip(('bias', 'temb', 'res', 'div'), (m & 1, m & 2, m & 4, m & 8)) if on) for m in range(16)]


@pytest.mark.parametrize('opts', OPTS, ids=lambda o: '+'.join(sorted(o)) or 'bare')
def test_forward_halo_options(hip_lib, opts):
  """gemm_halo_kernel<16, EpFwd>, staged addends: each of bias / temb / res / out_div on and off; 32 dead rows per tile"""
  _forward(hip_lib, 96, 32, 96, 16, 16, 3, 'h16', opts)


@pytest.mark.parametrize('opts', [frozenset(), frozenset(('bias', 'temb', 'res', 'div'))], ids=['bare', 'full'])
def test_forward_unsplit_half_dead_tile(hip_lib, opts):
  """x2d::gemm_kernel<9, 128, EpFwd>: 8 x 8 maps, two row tiles (160 rows), the last pixel tile half dead"""
  _forward(hip_lib, 191, 32, 160, 8, 8, 3, 'g', opts)


@pytest.mark.parametrize('N,HW,opts', [(1536, 4, ('temb',)), (1536, 4, ('bias', 'temb', 'res', 'div')), (6144, 2, ('temb',)),
                                       (6144, 2, ('bias', 'temb', 'res', 'div')), (6144, 2, ('res',))],
                         ids=['4x4-staged-temb', '4x4-staged-full', '2x2-unstaged-temb', '2x2-unstaged-full', '2x2-no-temb-res'])
def test_forward_temb_across_images(hip_lib, N, HW, opts):
  """a 128-pixel tile over 8 images (4 x 4 maps: staged temb) and over 32 (2 x 2: more than TEMB_IMGS, the unstaged strip);
  without temb the 2 x 2 tile takes the staged strip again"""
  _forward(hip_lib, N, 32, 128, HW, HW, 3, 'g', frozenset(opts))


@pytest.mark.parametrize('opts', [frozenset(), frozenset(('bias', 'temb', 'res', 'div'))], ids=['bare', 'full'])
def test_forward_ksplit_short_last_split(hip_lib, opts):
  """EpSlab + slab sum: one 8 x 8 tile of 128 pixels, 27 chunks in splits of 14 + 13"""
  _forward(hip_lib, 2, 96, 96, 8, 8, 3, 'ks', opts, splits=(14, 13))


@pytest.mark.parametrize('opts', [frozenset(), frozenset(('bias', 'temb', 'res', 'div'))], ids=['bare', 'full'])
def test_forward_1x1_two_sources_f32(hip_lib, opts):
  """x2::gemm_kernel<ActLoader<true, 1>, EpFwd>: the f32-operand entry, sources of 64 + 32 channels, ragged last tile"""
  _forward(hip_lib, 51, 96, 160, 12, 20, 1, None, opts, entry='f32', S1=64)


BETAS = [(0.0, 0.0), (1.0, 0.0), (0.5, 1.0)]


@pytest.mark.parametrize('beta', BETAS, ids=lambda b: f'beta{b[0]:g}_{b[1]:g}')
@pytest.mark.parametrize('missing', [None, 'dx2', 'dx1'], ids=['both', 'dx2-null', 'dx1-null'])
@pytest.mark.parametrize('C1,C2', [(64, 32), (48, 48)], ids=['64+32', '48+48'])
def test_dgrad_two_destinations(hip_lib, C1, C2, missing, beta):
  """gemm_halo_kernel<16, EpDgrad>: rows [0, C1) to dx1 and [C1, 96) to dx2 (32 dead rows), either destination NULL,
  accumulation on neither, one or both; the old gradients are exact (dyadic), and NaN where beta is 0.  48 + 48: the
  destinations meet inside a 32-row strip, which then serves both."""
  lib, d = hip_lib, dev_of(hip_lib)
  N, H, W, K, Kc = 96, 16, 16, 3, 32
  M = C1 + C2
  dy, w, Wg, acc = _operands(N, Kc, M, H, W, K, 0, True)
  _assert_form(lib, 1, (C1, C2, N, H, W, Kc), K, 'h16')
  dx0 = _dyadic((N, M, H, W), 4, 5)
  for rows, b in ((slice(0, C1), beta[0]), (slice(C1, M), beta[1])):
    if b == 0.0:
      dx0[:, rows] = np.nan           # never read
  nb = int(lib.conv2d_dgrad_ws_bytes(C1, C2, N, H, W, Kc, K, K, 1, K // 2))
  g_dy, g_w, g_ws = Guarded(dy, d), Guarded(w, d), Guarded(_bytes(nb), d)
  g1 = None if missing == 'dx1' else Guarded(np.ascontiguousarray(dx0[:, :C1]), d)
  g2 = None if missing == 'dx2' else Guarded(np.ascontiguousarray(dx0[:, C1:]), d)
  planes, rec = _planes_of(lib, g_dy, dy, d)
  call(lib, 'conv2d_dgrad_pl_f32', planes, rec, g_w.view, 0, g1.view if g1 else None, C1, beta[0],
       g2.view if g2 else None, C2, beta[1], 0.5, N, H, W, Kc, K, K, None, g_ws.view, nb)
  if lib.is_device:
    torch.cuda.synchronize()
  what = f'dgrad {C1}+{C2} {missing} {beta}'
  for g in (g_dy, g_w, g_ws, g1, g2):
    if g is not None:
      g.check(what)
  t = cr.three_term(cr.problem(True, dy, Wg, K * K, alpha=0.5, C1=C1, beta=beta, dx0=dx0), acc=acc)
  for g, rows in ((g1, slice(0, C1)), (g2, slice(C1, M))):
    if g is not None:
      _equal(g.view.cpu().numpy(), t['out'][:, rows], t['lolo'][:, rows], lib, f'{what} rows {rows}')


@pytest.mark.parametrize('beta', BETAS, ids=lambda b: f'beta{b[0]:g}_{b[1]:g}')
@pytest.mark.parametrize('C1,C2', [(16, 16), (40, 24), (3, 0)], ids=['16+16', '40+24', '3'])
def test_dgrad_f32_kernel_unaligned_sources(hip_lib, C1, C2, beta):
  """igemm::kernel<.., EpDgrad> (no scratch: the f32-operand MFMA kernel, which keeps the element strip): a first source that
  is no multiple of 32 channels, so one 32-row strip serves both destinations.  INTEGER operands (l = 0: the full product is exact on any path), old
  gradients dyadic, NaN where beta is 0."""
  lib, d = hip_lib, dev_of(hip_lib)
  N, H, W, K, Kc = 3, 8, 8, 3, 16
  M = C1 + C2
  g = np.random.default_rng(7)
  dy = g.integers(-2, 3, (N, Kc, H, W)).astype(np.float32)
  w = g.integers(-2, 3, (Kc, M, K, K)).astype(np.float32)
  dy.flat[5], w.flat[7] = 2.0, 2.0
  Wg = cr.gemm_weights(w, 0, M, Kc, K, True)
  dx0 = _dyadic((N, M, H, W), 4, 5)
  for rows, b in ((slice(0, C1), beta[0]), (slice(C1, M), beta[1])):
    if b == 0.0:
      dx0[:, rows] = np.nan
  g_dy, g_w = Guarded(dy, d), Guarded(w, d)
  g1 = Guarded(np.ascontiguousarray(dx0[:, :C1]), d)
  g2 = Guarded(np.ascontiguousarray(dx0[:, C1:]), d) if C2 else None
  call(lib, 'conv2d_dgrad_f32', g_dy.view, g_w.view, 0, g1.view, C1, beta[0], g2.view if g2 else None, C2, beta[1], 0.5,
       N, H, W, Kc, H, W, K, K, 1, K // 2, None, 0)
  if lib.is_device:
    torch.cuda.synchronize()
  what = f'dgrad f32 {C1}+{C2} {beta}'
  for gd in (g_dy, g_w, g1, g2):
    if gd is not None:
      gd.check(what)
  t = cr.three_term(cr.problem(True, np.pad(dy, ((0, 0), (0, 16), (0, 0), (0, 0))), np.pad(Wg, ((0, 0), (0, 16), (0, 0))), K * K,
                               alpha=0.5, C1=C1, beta=beta, dx0=dx0))
  assert not t['lolo'].any()
  for gd, rows in ((g1, slice(0, C1)), (g2, slice(C1, M))):
    if gd is not None:
      _equal(gd.view.cpu().numpy(), t['out'][:, rows], t['lolo'][:, rows], lib, f'{what} rows {rows}')


def test_wgrad_1x1_dead_columns(hip_lib):
  """x2::wgemm_kernel<.., EpWgrad> + the slab reduction: dw [160, 80] += 0.5 sum dy x; two row tiles, the second with 32
  live rows, 48 dead columns; dw starts exact.  Exact model: dy_h (x_h + x_l) + dy_l x_h summed over 512 pixels."""
  lib, d = hip_lib, dev_of(hip_lib)
  N, H, W, Cin, Cout = 2, 16, 16, 80, 160
  x, dy = cr.exact_tensor((N, Cin, H, W), 1, 1), cr.exact_tensor((N, Cout, H, W), 1, 2)
  dw0 = _dyadic((Cout, Cin, 1, 1), 4, 5)
  nb = int(lib.conv2d_wgrad_ws_bytes(Cin, 0, N, Cout, H, W, 1, 1))
  if lib.is_device:
    assert int(lib.conv2d_variant(2, Cin, 0, N, H, W, Cout, H, W, 1, 1, 1, 0, 0)) == 5, 'not the split weight gradient'
  g_x, g_dy, g_dw = Guarded(x, d), Guarded(dy, d), Guarded(dw0, d)
  g_ws = Guarded(torch.full((max(nb // 4, 4),), float(SENT)), d)
  call(lib, 'conv2d_wgrad_f32', g_x.view, Cin, None, 0, g_dy.view, g_dw.view, 0, 0.5, g_ws.view, nb, N, H, W, Cout,
       H, W, 1, 1, 1, 0)
  if lib.is_device:
    torch.cuda.synchronize()
  for g in (g_x, g_dy, g_dw, g_ws):
    g.check('wgrad')
  sx, sd = cr.pow2_scale_of(2.0), cr.pow2_scale_of(2.0)
  xh, xl, _ = cr.split(x, sx)
  dh, dl, _ = cr.split(dy, sd)
  xh, xl, dh, dl = (t.astype(np.float64).transpose(1, 0, 2, 3).reshape(t.shape[1], -1) for t in (xh, xl, dh, dl))
  three = (dh @ (xh + xl).T + dl @ xh.T) / (sx * sd)
  lolo = (dl @ xl.T) / (sx * sd)
  want = dw0.reshape(Cout, Cin).astype(np.float64) + 0.5 * three
  _equal(g_dw.view.cpu().numpy().reshape(Cout, Cin), want, 0.5 * lolo, lib, 'wgrad 1x1')
