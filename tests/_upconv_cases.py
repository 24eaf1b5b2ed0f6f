"""The FIR-upsampling convolution (csrc/upconv.hip) on every launch form: cases, the float64 reference on the operands the
kernels receive, the per-element rounding bound, a restatement of the host's form rules and the guarded launch sequence
(tests/test_gpu_upconv_forms.py on the HIP library, tests/test_upconv_cases_cpu.py without a GPU).

Reference.  tests/_upconv_ref.py's forward_taps / grads_taps in float64 torch on the CPU, from the float32 operands widened:
the float32 taps, out_div rounded to float32, alpha and beta exact in float32.

Bound (derived, never fitted).  Every output is multilinear in its operands, so B, the sum of the absolute terms of an
element, is the same reference on |x|, |w|, |fir|, |bias|, |res|, |dy|, |dx0|, |dw0|.  Each element is held to
  |err| <= k 2^-24 B + 2^-126
with k the roundings on that element's path.  The MFMA is bit-equal to an fmaf chain in k order (igemm.h), the FIR is fmaf
(up_fir_kernel), and a chain of n fused multiply-adds is within n 2^-24 of its sum of absolute terms in any order:
  y    Cin ((K+1)/2)^2   the longest parity's chain (AUpFwd / BUpFwd: k = (ci, s, t), ty tx <= ((K+1)/2)^2 taps a channel)
       + KT^2            up_fir_kernel: KT rows of KT fmaf
       + 4               r += bv; r += res; inv = 1.f / out_div (launch_fir); r *= inv
  du   KT^2              up_fir_kernel with no bias, res or division
  dx   Cout K^2          the chain over k = (co, t') of AUpDg9 / AUpDg1 with BUpDg
       + KT^2            the roundings du carries
       + 3               EpUpDg: beta * dx, alpha * acc, their sum
  dw   N H W             the chains of all slabs together (AUpWg / BUpWg, k = the pixels)
       + splits          up_reduce_kernel: sum += part[z]
       + KT^2            du
       + 2               alpha * sum, dw +=
The sums of the weight gradient are also held on their own: dw0 enters through the last addition alone, so
  |dw - dw0 - alpha S| <= k 2^-24 |alpha| B_S + 2^-24 |dw|        (the half ulp of the result that dw0 brings in).

Data.  Operands are randn; the taps are randn(KT, KT), neither separable nor symmetric (a symmetric FIR hides a flipped or
transposed tap index and an exchanged pad); one case keeps the model's normalised (1, 3, 3, 1).  `scaled` cases multiply
image n of x, res and dy by 10^e(n), e spread over [-2, 2]: the per-element bound holds the smallest image to its own scale.

Forms.  big_tile, wg_plan and the parity loop of stk_upconv2d_fwd_f32 restated below; forms(case) lists what a case
reaches and REQUIRED what the table must reach.  The library's only queries are the two workspace sizes: the GPU test
checks `splits` and the size of u against them; tile widths are as good as the reading they were written from.
"""
import collections
import functools

import torch

import _upconv_ref as ur
from _stream_util import Guarded, U

TINY = 2.0 ** -126
STK_EINVAL, STK_EUNSUPPORTED = -1, -3
SQRT2 = float(torch.tensor(2.0 ** 0.5, dtype=torch.float32))          # out_div as the kernel receives it

# ---- cases ------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'name N Cin Cout H W K KT pad0 taps bias res div scaled a_dx a_dw')


def model_pad0(K, KT):
  """pad0 of upsample_conv_2d: p = (KT - 2) - (K - 1), pad = ((p + 1) // 2 + 1, p // 2 + 1)."""
  return ((KT - 2) - (K - 1) + 1) // 2 + 1


def _c(dims, pad0=None, taps='randn', bias=True, res=True, div=True, scaled=False, a_dx=(1.0, 0.75), a_dw=(0.75, 1.0)):
  """dims = (N, Cin, Cout, H, W, K, KT).  a_dx: alpha of the data gradient at beta = 0 (into a NaN-filled dx) and at beta = 0.5;
  a_dw: alpha of the weight gradient from the du left behind and from dy."""
  N, Cin, Cout, H, W, K, KT = dims
  p0 = model_pad0(K, KT) if pad0 is None else pad0
  name = f'b{N}_{Cin}to{Cout}_{H}x{W}_k{K}_t{KT}' + ('' if pad0 is None else f'_p{pad0}') + ('_1331' if taps == '1331' else '')
  return Case(name, N, Cin, Cout, H, W, K, KT, p0, taps, bias, res, SQRT2 if div else 1.0, scaled, a_dx, a_dw)


CASES = [
  # forward 128-tiles with TAPS 4 / 2 / 1 (206 / 195 / 195 / 192 tiles); weight gradient 64-tile, 15 slabs of 832, the last 640
  _c((12, 8, 256, 32, 32, 3, 3), bias=False, res=False, div=False, a_dx=(-1.25, 1.0)),
  # forward 128-tile at K = 1 (memset, the even-even parity only); KT = 1
  _c((12, 8, 256, 32, 32, 1, 1), res=False),
  # forward 128-tile with M / N tails and k tails 16 / 8 / 4 after full chunks; 2W % 4 = 2; 15 slabs, the last 755 (tail 19)
  _c((13, 36, 200, 31, 33, 3, 4), scaled=True, bias=False),
  # data gradient 128-tile, K = 3, two full 36-chunks
  _c((12, 256, 8, 32, 32, 3, 3), div=False, a_dw=(1.0, 0.75)),
  # data gradient 128-tile, K = 1, k tail 8
  _c((12, 256, 8, 32, 32, 1, 2), bias=False, res=False, div=False),
  # data gradient 128-tile with M tail 72, N tail 115, chunks 36 + 27
  _c((13, 200, 7, 31, 33, 3, 4), scaled=True, res=False, a_dx=(0.75, -1.25)),
  # data gradient 128-tile at K = 1 with M / N tails and a k tail after a full chunk
  _c((13, 200, 37, 31, 33, 1, 3), bias=False, div=False),
  # weight gradient 128-tile, 2 slabs of 576, the last 516 (tail 4)
  _c((7, 96, 96, 12, 13, 3, 4), pad0=2),
  # weight gradient 128-tile at K = 3, one slab of 189 pixels (tail 29)
  _c((3, 96, 100, 9, 7, 3, 1), res=False, div=False),
  # weight gradient 128-tile with Cout / Cin tails, several even slabs
  _c((8, 97, 100, 16, 16, 3, 2), res=False, div=False),
  # weight gradient 128-tile at K = 1: one slab with pixel tail 30; two even slabs; two slabs, the last 539 (tail 27)
  _c((2, 384, 384, 9, 7, 1, 3), bias=False),
  _c((4, 257, 260, 16, 16, 1, 1), bias=False, div=False),
  _c((3, 257, 260, 19, 19, 1, 2)),
  # weight gradient 64-tile, 2 slabs with a short last; data gradient chunk tail 18 after 17 full chunks; forward k tails 16 / 8
  _c((7, 40, 70, 12, 13, 3, 1), scaled=True, bias=False, div=False),
  # weight gradient 128-tile, 10 slabs with the last 507 (tail 27); forward k tails 16 / 8 / 4 after full chunks on 64-tiles
  _c((5, 100, 97, 33, 31, 3, 2), scaled=True),
  # weight gradient 64-tile at K = 1: one slab; even slabs; a short last slab
  _c((3, 40, 70, 5, 7, 1, 2), res=False),
  _c((4, 70, 40, 32, 32, 1, 4), pad0=0, bias=False, res=False),
  _c((5, 65, 33, 21, 19, 1, 3), div=False),
  # weight gradient 64-tile at K = 3, even slabs
  _c((4, 40, 70, 16, 16, 3, 3), pad0=0, res=False),
  # map edges: one pixel, one row, one column (K = 1 and K = 3), H != W both odd are above
  _c((2, 5, 6, 1, 1, 3, 4)),
  _c((3, 33, 65, 1, 7, 3, 3), bias=False, res=False, div=False),
  _c((3, 65, 33, 5, 1, 1, 4), pad0=3, res=False),
  _c((2, 6, 5, 3, 1, 3, 2), bias=False),
  _c((2, 6, 5, 1, 1, 1, 1), pad0=0, div=False),
  # every pad0 of 0 .. KT - 1 at KT = 4 (the model's are 1 at K = 3, 2 at K = 1) and at KT = 3, KT = 2
  _c((2, 5, 6, 6, 5, 3, 4), pad0=0, div=False),
  _c((2, 5, 6, 6, 5, 3, 4), pad0=3, bias=False),
  _c((2, 5, 6, 5, 6, 1, 4), res=False),
  _c((2, 5, 6, 5, 6, 3, 3), pad0=2),
  _c((2, 5, 6, 5, 6, 3, 3), pad0=1, bias=False, res=False, div=False),
  _c((2, 5, 6, 5, 6, 1, 2), pad0=0, bias=False),
  # one even case of the earlier table, with the model's normalised taps
  _c((128, 64, 96, 8, 8, 3, 4), taps='1331'),
]
IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
SHORT = 40            # the contraction length (in channels) up to which a case is expected to show a loss of precision


# ---- the host's form rules, restated -----------------------------------------------------------------------------------
def cdiv(a, b):
  return -(-a // b)


def big_tile(M, N):
  """upconv.hip big_tile(M, N, 1): 128 x 128 tiles when they still give every CU work."""
  return M >= 96 and N >= 96 and cdiv(M, 128) * cdiv(N, 128) >= 192


def wg_plan(c):
  """upconv.hip wg_plan -> (tile, splits, k_per_split)."""
  Kp = c.N * c.H * c.W
  KK = c.K * c.K
  big = c.Cout >= 96 and c.Cin >= 96 and cdiv(c.Cout, 128) * cdiv(c.Cin, 128) * KK >= 9
  T = 128 if big else 64
  tiles = cdiv(c.Cout, T) * cdiv(c.Cin, T) * KK
  chunks = (Kp + 31) // 32
  splits = max(min(cdiv(512, tiles), chunks // 16), 1)
  kps = cdiv(chunks, splits) * 32
  return T, cdiv(Kp, kps), kps


def parities(c):
  """The launches of stk_upconv2d_fwd_f32's parity loop: [(py, px, TAPS, PH, PW, tile)]."""
  UH, UW = 2 * c.H - 2 + c.K, 2 * c.W - 2 + c.K
  out = []
  for py in (0, 1):
    for px in (0, 1):
      ty = (c.K + 1) // 2 if py == 0 else (c.K - 1) // 2
      tx = (c.K + 1) // 2 if px == 0 else (c.K - 1) // 2
      PH = (UH + 1) // 2 if py == 0 else UH // 2
      PW = (UW + 1) // 2 if px == 0 else UW // 2
      if ty * tx == 0 or PH * PW == 0:
        continue
      out.append((py, px, ty * tx, PH, PW, 128 if big_tile(c.Cout, c.N * PH * PW) else 64))
  return out


def dgrad_tile(c):
  return 128 if big_tile(c.Cin, c.N * c.H * c.W) else 64


def forms(c):
  """The set of launch forms case c reaches (strings, the vocabulary of REQUIRED)."""
  f = set()
  for py, px, taps, PH, PW, T in parities(c):
    base = f'fwd K{c.K} taps{taps} tile{T}'
    f.add(base)
    if c.Cout % T:
      f.add(base + ' M-tail')
    if (c.N * PH * PW) % T:
      f.add(base + ' N-tail')
    if (c.Cin * taps) % 32 and c.Cin * taps > 32:
      f.add(base + ' k-tail after a full chunk')
  T = dgrad_tile(c)
  base = f'dgrad K{c.K} tile{T}'
  f.add(base)
  if c.Cin % T:
    f.add(base + ' M-tail')
  if (c.N * c.H * c.W) % T:
    f.add(base + ' N-tail')
  KC = 36 if c.K == 3 else 32
  if (c.Cout * c.K * c.K) % KC and c.Cout * c.K * c.K > KC:
    f.add(base + ' k-tail after a full chunk')
  T, splits, kps = wg_plan(c)
  base = f'wgrad K{c.K} tile{T}'
  Kp = c.N * c.H * c.W
  last = Kp - (splits - 1) * kps
  if splits == 1:
    f.add(base + ' one slab')
    if Kp % 32:
      f.add(base + ' one slab, pixel tail')
  elif last == kps:
    f.add(base + ' even slabs')
  elif last % 32:
    f.add(base + ' short last slab, not a multiple of 32')
  if c.Cout % T and c.Cin % T:
    f.add(base + ' Cout and Cin tails')
  KT, w4 = c.KT, (2 * c.W) % 4
  f.add(f'fir KT{KT} forward 2W%4={w4}')
  f.add(f'fir KT{KT} adjoint')
  for what, on in (('bias', c.bias), ('res', c.res), ('div', c.div != 1.0)):
    f.add(f'fir KT{KT} forward {"with" if on else "without"} {what}')
  f.add(f'fir KT{KT} pad0={c.pad0}' + (' (the model\'s)' if c.pad0 == model_pad0(c.K, KT) else ''))
  if c.H == 1 and c.W == 1:
    f.add(f'map 1x1 K{c.K}')
  elif c.H == 1 and c.W % 2:
    f.add('map H=1, W odd')
  elif c.W == 1:
    f.add(f'map W=1 K{c.K}')
  elif c.H != c.W and c.H % 2 and c.W % 2:
    f.add('map H!=W, both odd')
  if c.scaled:
    f.add('scaled, short' if min(c.Cin, c.Cout) <= SHORT else 'scaled')
  f.add('taps ' + c.taps)
  for a in c.a_dx:
    f.add(f'dgrad alpha {a}')
  for a in c.a_dw:
    f.add(f'wgrad alpha {a}')
  return f


def _required():
  R = set()
  for T in (64, 128):
    for taps in (4, 2, 1):
      base = f'fwd K3 taps{taps} tile{T}'
      R |= {base, base + ' M-tail', base + ' N-tail', base + ' k-tail after a full chunk'}
    R.add(f'fwd K1 taps1 tile{T}')
    for K in (3, 1):
      base = f'dgrad K{K} tile{T}'
      R |= {base, base + ' M-tail', base + ' N-tail', base + ' k-tail after a full chunk'}
      base = f'wgrad K{K} tile{T}'
      R |= {base + ' one slab', base + ' even slabs', base + ' short last slab, not a multiple of 32', base + ' Cout and Cin tails'}
  R.add('wgrad K1 tile128 one slab, pixel tail')
  for KT in (1, 2, 3, 4):
    R |= {f'fir KT{KT} forward 2W%4=0', f'fir KT{KT} forward 2W%4=2', f'fir KT{KT} adjoint'}
    for what in ('bias', 'res', 'div'):
      R |= {f'fir KT{KT} forward with {what}', f'fir KT{KT} forward without {what}'}
    for K in (1, 3):
      R.add(f'fir KT{KT} pad0={model_pad0(K, KT)} (the model\'s)')
  for KT in (2, 3, 4):
    for p in range(KT):
      R.add(f'fir KT{KT} pad0={p}' + (' (the model\'s)' if p in (model_pad0(1, KT), model_pad0(3, KT)) else ''))
  R |= {'map 1x1 K3', 'map 1x1 K1', 'map H=1, W odd', 'map W=1 K1', 'map W=1 K3', 'map H!=W, both odd'}
  R |= {'scaled, short', 'scaled', 'taps randn', 'taps 1331'}
  R |= {f'dgrad alpha {a}' for a in (1.0, 0.75, -1.25)} | {f'wgrad alpha {a}' for a in (1.0, 0.75)}
  return R


REQUIRED = _required()


# ---- rounding counts ---------------------------------------------------------------------------------------------------
def counts(c):
  """k of y, du, dx, dw and of the weight gradient's sums (the module text has the derivation)."""
  kt2 = c.KT * c.KT
  splits = wg_plan(c)[1]
  return {'y': c.Cin * ((c.K + 1) // 2) ** 2 + kt2 + 4, 'du': kt2, 'dx': c.Cout * c.K * c.K + kt2 + 3,
          'dw': c.N * c.H * c.W + splits + kt2 + 2}


# ---- operands ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def inputs(name):
  """The float32 operands of a case on the CPU (cached, never modified): x, w, fir, bias, res, dy, dx0, dw0."""
  c = BY_NAME[name]
  g = torch.Generator().manual_seed(7000 + IDS.index(name))
  rn = lambda *s: torch.randn(*s, generator=g)
  scale = torch.ones(c.N, 1, 1, 1)
  if c.scaled:
    e = torch.linspace(-2.0, 2.0, c.N)
    # neighbouring images far apart; the last image is the largest, so the weight gradient's last (short) slab carries weight
    order = [i // 2 if i % 2 == 0 else c.N - 1 - i // 2 for i in range(c.N)]
    order = [c.N - 1 - o for o in reversed(order)]
    scale = (10.0 ** e[order]).view(c.N, 1, 1, 1)
  t = {'x': rn(c.N, c.Cin, c.H, c.W) * scale, 'w': rn(c.Cout, c.Cin, c.K, c.K)}
  if c.taps == '1331':
    t['fir'] = ur.taps_pad((1, 3, 3, 1), c.K, dtype=torch.float32)[0].contiguous()
    assert t['fir'].shape[0] == c.KT
  else:
    t['fir'] = rn(c.KT, c.KT)
  t['bias'] = rn(c.Cout) if c.bias else None
  t['res'] = rn(c.N, c.Cout, 2 * c.H, 2 * c.W) * scale if c.res else None
  t['dy'] = rn(c.N, c.Cout, 2 * c.H, 2 * c.W) * scale
  t['dx0'] = rn(c.N, c.Cin, c.H, c.W) * scale
  t['dw0'] = rn(c.Cout, c.Cin, c.K, c.K)
  return t


def smallest_image(name):
  """The image of a scaled case with the smallest scale."""
  x = inputs(name)['x'].double()
  return int(x.pow(2).mean((1, 2, 3)).argmin())


# ---- reference and bound -------------------------------------------------------------------------------------------------
BETA = 0.5
OUTPUTS = ('y', 'du', 'dx_b0', 'dx_acc', 'dw_du', 'dw_dy')


def _d(t):
  return None if t is None else t.double()


def evaluate(c, t, dtype=torch.float64):
  """Every output of the launch sequence from operands t, in `dtype` torch on the CPU; with the absolute values of the
  operands (and of alpha, beta) this is B.  S is the weight gradient's plain sum (alpha = 1, dw0 = 0)."""
  cv = lambda v: None if v is None else v.to(dtype)
  x, w, kf, dy = cv(t['x']), cv(t['w']), cv(t['fir']), cv(t['dy'])
  y, u = ur.forward_taps(x, w, kf, c.pad0, cv(t['bias']), cv(t['res']), torch.tensor(c.div, dtype=dtype))
  dx, dw, du = ur.grads_taps(x, w, dy, kf, c.pad0)
  a = t.get('alphas', (c.a_dx, c.a_dw))
  return {'y': y, 'u': u, 'du': du, 'dx_b0': a[0][0] * dx, 'dx_acc': BETA * cv(t['dx0']) + a[0][1] * dx,
          'dw_du': cv(t['dw0']) + a[1][0] * dw, 'dw_dy': cv(t['dw0']) + a[1][1] * dw, 'S': dw}


def magnitudes(c, t):
  ta = {k: (None if v is None else v.abs()) for k, v in t.items()}
  ta['alphas'] = (tuple(abs(a) for a in c.a_dx), tuple(abs(a) for a in c.a_dw))
  return evaluate(c, ta)


@functools.lru_cache(maxsize=2)
def reference(name):
  """(want, B): the float64 outputs of a case and their sums of absolute terms, computed once and shared."""
  c, t = BY_NAME[name], inputs(name)
  return evaluate(c, t), magnitudes(c, t)


def bounds(c, mag):
  """The per-element bound of every output, float64 tensors."""
  k = counts(c)
  kk = {'y': k['y'], 'du': k['du'], 'dx_b0': k['dx'], 'dx_acc': k['dx'], 'dw_du': k['dw'], 'dw_dy': k['dw']}
  return {o: kk[o] * U * mag[o] + TINY for o in OUTPUTS}


def locate(c, out, flat):
  """Where element `flat` of output `out` lies: its index, the parity of the map it belongs to and its GEMM tile."""
  if out == 'y':
    shape = (c.N, c.Cout, 2 * c.H, 2 * c.W)
  elif out in ('du', 'u'):
    shape = (c.N, c.Cout, 2 * c.H - 2 + c.K, 2 * c.W - 2 + c.K)
  elif out.startswith('dx'):
    shape = (c.N, c.Cin, c.H, c.W)
  else:
    shape = (c.Cout, c.Cin, c.K, c.K)
  idx, r = [], flat
  for s in reversed(shape):
    idx.append(r % s)
    r //= s
  idx = tuple(reversed(idx))
  if out in ('y', 'u'):              # for y: the element of u under it (the FIR mixes the parities around it)
    b, co, oy, ox = idx
    where = f'parity ({oy % 2}, {ox % 2})'
    for py, px, taps, PH, PW, T in parities(c):
      if (py, px) == (oy % 2, ox % 2):
        n = b * PH * PW + min(oy // 2, PH - 1) * PW + min(ox // 2, PW - 1)
        where += f', TAPS {taps}, {T}-tile (m {co // T}, n {n // T}) of that parity of u'
  elif out == 'du':
    where = f'parity ({idx[2] % 2}, {idx[3] % 2}), quad {idx[3] // 4} of row {idx[2]}'
  elif out.startswith('dx'):
    b, ci, i, j = idx
    T = dgrad_tile(c)
    where = f'{T}-tile (m {ci // T}, n {(b * c.H * c.W + i * c.W + j) // T})'
  else:
    T, splits, kps = wg_plan(c)
    where = f'tap {idx[2] * c.K + idx[3]}, {T}-tile (m {idx[0] // T}, n {idx[1] // T}), {splits} slabs of {kps}'
  return f'index {idx}, {where}'


def check(c, out, got, want, bnd, show=True):
  """|got - want| <= bnd element by element, nothing excluded, no NaN -> the worst err / bound."""
  g = got.detach().cpu().double().reshape(-1)
  w, b = want.reshape(-1), bnd.reshape(-1)
  assert g.shape == w.shape, (c.name, out, got.shape, want.shape)
  nonfinite = (~torch.isfinite(g)).nonzero()
  assert nonfinite.numel() == 0, f'{c.name} {out}: {nonfinite.numel()} non-finite elements, the first at {locate(c, out, int(nonfinite[0]))}'
  ratio = (g - w).abs() / b
  worst = int(ratio.argmax())
  r = float(ratio[worst])
  if show:
    print(f'  {c.name} {out}: worst err / bound {r:.3g}')
  assert r <= 1.0, f'{c.name} {out}: err / bound {r:.3g} ({int((ratio > 1).sum())} elements over) at {locate(c, out, worst)}: ' \
                   f'got {float(g[worst])!r}, want {float(w[worst])!r}, bound {float(b[worst]):.3g}'
  return r


def check_sums(c, out, got, alpha, want, mag, show=True):
  """The sums of the weight gradient on their own scale: |dw - dw0 - alpha S| <= k u |alpha| B_S + u |dw|."""
  dw0 = inputs(c.name)['dw0'].double()
  g = got.detach().cpu().double()
  bnd = counts(c)['dw'] * U * abs(alpha) * mag['S'] + U * g.abs() + TINY
  ratio = ((g - dw0 - alpha * want['S']).abs() / bnd).reshape(-1)
  worst = int(ratio.argmax())
  r = float(ratio[worst])
  if show:
    print(f'  {c.name} {out} sums: worst err / bound {r:.3g}')
  assert r <= 1.0, f'{c.name} {out} sums: err / bound {r:.3g} at {locate(c, out, worst)}'
  return r


# ---- the launch sequence -------------------------------------------------------------------------------------------------
def _nan_like(shape):
  return torch.full(shape, float('nan'), dtype=torch.float32)


def run(lib, c, dev):
  """The sequence of one case through the C ABI on fresh guarded buffers: forward; the data gradient from dy (du_valid = 0,
  beta = 0 into a NaN-filled dx); the data gradient (beta = 0.5) and the weight gradient from the du it left (du_valid = 1,
  dy and fir NULL); the weight gradient from dy into a fresh NaN-filled du.  Returns the outputs on the CPU; the guards, the
  workspace sizes against the restated plan and du's bits under du_valid = 1 are asserted here."""
  from _ufd_cases import guarded_in
  from _util import call
  t = inputs(c.name)
  d = {k: (None if v is None else guarded_in(v, dev)) for k, v in t.items() if k not in ('dx0', 'dw0')}
  dims = (c.N, c.H, c.W, c.Cin, c.Cout, c.K, c.KT)
  UH, UW = 2 * c.H - 2 + c.K, 2 * c.W - 2 + c.K
  T, splits, kps = wg_plan(c)
  nb_u, nb_wg = int(lib.upconv2d_ws_bytes(0, *dims)), int(lib.upconv2d_ws_bytes(2, *dims))
  assert nb_u == 4 * c.N * c.Cout * UH * UW, (c.name, nb_u)
  assert nb_wg == splits * 4 * c.Cout * c.Cin * c.K * c.K, f'{c.name}: the library plans {nb_wg / (4 * c.Cout * c.Cin * c.K * c.K)} slabs, the restatement {splits}'
  assert int(lib.upconv2d_ws_bytes(1, *dims)) == 0
  G = {}

  def buf(name, start):
    G[name] = Guarded(start, dev)          # 8 sentinels before and after: the trailing guard starts exactly at the last byte + 1
    return G[name].view

  y = buf('y', _nan_like((c.N, c.Cout, 2 * c.H, 2 * c.W)))
  ws_u = buf('ws_u', _nan_like((nb_u // 4,)))
  call(lib, 'upconv2d_fwd_f32', d['x'], d['w'], d['fir'], d['bias'], d['res'], c.div, y, *dims, c.pad0, ws_u, nb_u)
  du = buf('du', _nan_like((c.N, c.Cout, UH, UW)))
  dx_b0 = buf('dx_b0', _nan_like((c.N, c.Cin, c.H, c.W)))
  call(lib, 'upconv2d_dgrad_f32', d['dy'], d['w'], d['fir'], du, 0, dx_b0, 0.0, c.a_dx[0], *dims, c.pad0)
  du_left = du.clone()
  dx_acc = buf('dx_acc', t['dx0'])
  call(lib, 'upconv2d_dgrad_f32', None, d['w'], None, du, 1, dx_acc, BETA, c.a_dx[1], *dims, c.pad0)
  dw_du = buf('dw_du', t['dw0'])
  ws_a = buf('ws_a', _nan_like((nb_wg // 4,)))
  call(lib, 'upconv2d_wgrad_f32', d['x'], None, None, du, 1, dw_du, c.a_dw[0], *dims, c.pad0, ws_a, nb_wg)
  assert torch.equal(du.view(torch.int32), du_left.view(torch.int32)), f'{c.name}: du was written under du_valid = 1'
  du2 = buf('du2', _nan_like((c.N, c.Cout, UH, UW)))
  dw_dy = buf('dw_dy', t['dw0'])
  ws_b = buf('ws_b', _nan_like((nb_wg // 4,)))
  call(lib, 'upconv2d_wgrad_f32', d['x'], d['dy'], d['fir'], du2, 0, dw_dy, c.a_dw[1], *dims, c.pad0, ws_b, nb_wg)
  torch.cuda.synchronize()
  for name, g in G.items():
    g.check(f'{c.name} {name}')
  for k, v in d.items():
    if v is not None:
      assert torch.equal(v.cpu().view(torch.int32), t[k].view(torch.int32)), f'{c.name}: operand {k} was written'
  u = ws_u.view(c.N, c.Cout, UH, UW)
  out = {'y': y, 'u': u, 'du': du, 'dx_b0': dx_b0, 'dx_acc': dx_acc, 'dw_du': dw_du, 'dw_dy': dw_dy, 'du2': du2}
  return {k: v.cpu() for k, v in out.items()}
