"""tests/_upconv_cases.py without a GPU: the tap-array reference against the separable entries, against the header's formulas
written as loops over conv_transpose2d and against autograd of itself; the condition on the inputs (plain float32 passes the
bound on every element of every case); mutants of the reference, which must each exceed the bound at least five times over
on the cases meant to catch them; and the coverage of the launch forms by the case table."""
import pytest
import torch
import torch.nn.functional as F

import _upconv_cases as uc
import _upconv_ref as ur

MUTANT_FACTOR = 5.0
PIXEL_DW_MAX = 1024       # n^2 2^-24 = 1/16: one term of n is about 16 / 5 times five bounds of n 2^-24 (terms of equal size)


# ---- the case table ------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_form():
  assert len(set(uc.IDS)) == len(uc.IDS)
  reached = set()
  for c in uc.CASES:
    reached |= uc.forms(c)
  missing = sorted(uc.REQUIRED - reached)
  assert not missing, f'no case reaches: {missing}'
  # small: the largest map u is 52 MB, the largest contraction under 10^9 multiply-adds (a second of float64 on the CPU)
  for c in uc.CASES:
    assert 4 * c.N * c.Cout * (2 * c.H - 2 + c.K) * (2 * c.W - 2 + c.K) <= 53e6, c.name
    assert c.N * c.Cin * c.Cout * c.H * c.W * c.K * c.K <= 1e9, c.name


def test_restated_plans_of_the_chosen_cases():
  """The plans the table was chosen for, spelled out: a changed rule shows here before it silently moves a case elsewhere."""
  plan = lambda name: uc.wg_plan(uc.BY_NAME[name])
  assert plan('b12_8to256_32x32_k3_t3') == (64, 15, 832)                # the last slab 640
  assert plan('b13_36to200_31x33_k3_t4') == (64, 15, 896)               # the last 755 = 23 * 32 + 19
  assert plan('b7_96to96_12x13_k3_t4_p2') == (128, 2, 576)              # the last 516
  assert plan('b5_100to97_33x31_k3_t2') == (128, 10, 512)               # the last 507
  assert plan('b2_384to384_9x7_k1_t3') == (128, 1, 128)
  assert [p[5] for p in uc.parities(uc.BY_NAME['b12_8to256_32x32_k3_t3'])] == [128] * 4
  assert [p[2:5] for p in uc.parities(uc.BY_NAME['b2_6to5_1x1_k1_t1_p0'])] == [(1, 1, 1)]
  assert uc.dgrad_tile(uc.BY_NAME['b13_200to7_31x33_k3_t4']) == 128 and uc.dgrad_tile(uc.BY_NAME['b7_96to96_12x13_k3_t4_p2']) == 64


def test_scaled_cases_span_four_decades():
  for c in uc.CASES:
    if c.scaled:
      rms = uc.inputs(c.name)['x'].double().pow(2).mean((1, 2, 3)).sqrt()
      assert float(rms.max() / rms.min()) > 3e3, c.name


# ---- the reference -------------------------------------------------------------------------------------------------------
SMALL = [(2, 3, 4, 3, 5, 3, 4, 0), (2, 3, 4, 3, 5, 3, 4, 3), (1, 2, 3, 4, 3, 1, 4, 2), (2, 3, 2, 1, 1, 3, 3, 2), (2, 2, 3, 5, 1, 1, 1, 1),
         (1, 3, 2, 1, 5, 3, 2, 1), (2, 2, 2, 4, 4, 3, 1, 0), (1, 2, 2, 3, 3, 1, 2, 0)]      # N, Cin, Cout, H, W, K, KT, pad0


def _small(shape, seed=0):
  N, Cin, Cout, H, W, K, KT, pad0 = shape
  g = torch.Generator().manual_seed(seed)
  rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
  return rn(N, Cin, H, W), rn(Cout, Cin, K, K), rn(KT, KT), rn(Cout), rn(N, Cout, 2 * H, 2 * W), rn(N, Cout, 2 * H, 2 * W)


def _shift(t, dy, dx, OH, OW):
  """s[..., y, x] = t[..., y + dy, x + dx] for y < OH, x < OW, zero outside t."""
  m = max(abs(dy), abs(dx)) + max(OH, OW)
  p = F.pad(t, [m, m, m, m])
  return p[..., m + dy:m + dy + OH, m + dx:m + dx + OW]


@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_tap_reference_is_the_header(shape):
  """include/stk_upconv.h's formulas as sums of shifted maps, on conv_transpose2d's u: arbitrary taps, arbitrary pad0."""
  N, Cin, Cout, H, W, K, KT, pad0 = shape
  x, w, kf, bias, res, dy = _small(shape)
  y, u = ur.forward_taps(x, w, kf, pad0, bias, res, 1.5)
  ut = F.conv_transpose2d(x, torch.flip(w, [2, 3]).permute(1, 0, 2, 3), stride=2)
  assert ut.shape == u.shape and (u - ut).abs().max() <= 1e-12 * max(1.0, float(ut.abs().max()))
  want = sum(kf[KT - 1 - a, KT - 1 - b] * _shift(ut, a - pad0, b - pad0, 2 * H, 2 * W) for a in range(KT) for b in range(KT))
  want = (want + bias.view(1, -1, 1, 1) + res) / 1.5
  assert y.shape == want.shape and (y - want).abs().max() <= 1e-12 * float(want.abs().max())
  dx, dw, du = ur.grads_taps(x, w, dy, kf, pad0)
  c0 = KT - 1 - pad0
  du_w = sum(kf[a, b] * _shift(dy, a - c0, b - c0, 2 * H - 2 + K, 2 * W - 2 + K) for a in range(KT) for b in range(KT))
  assert du.shape == du_w.shape and (du - du_w).abs().max() <= 1e-12 * float(du_w.abs().max())
  # the two gather formulas, element by element
  dx_w, dw_w = torch.zeros_like(x), torch.zeros_like(w)
  for kh in range(K):
    for kw in range(K):
      for i in range(H):
        for j in range(W):
          g = du_w[:, :, 2 * i + K - 1 - kh, 2 * j + K - 1 - kw]                    # [N, Cout]
          dx_w[:, :, i, j] += g @ w[:, :, kh, kw]
          dw_w[:, :, kh, kw] += g.t() @ x[:, :, i, j]
  assert (dx - dx_w).abs().max() <= 1e-12 * float(dx_w.abs().max()) and (dw - dw_w).abs().max() <= 1e-12 * float(dw_w.abs().max())


@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_tap_reference_gradients_are_autograd_of_its_forward(shape):
  x, w, kf, bias, res, dy = _small(shape, seed=1)
  x.requires_grad_(True)
  w.requires_grad_(True)
  y, u = ur.forward_taps(x, w, kf, shape[7], bias, res)
  u.retain_grad()
  y.backward(dy)
  dx, dw, du = ur.grads_taps(x.detach(), w.detach(), dy, kf, shape[7])
  for got, want in ((du, u.grad), (dx, x.grad), (dw, w.grad)):
    assert got.shape == want.shape and (got - want).abs().max() <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize('K,k', [(3, (1, 3, 3, 1)), (1, (1, 3, 3, 1)), (3, (1, 1)), (1, (1, 1)), (3, (1, 2, 1)), (1, None)])
def test_tap_reference_agrees_with_the_separable_entries(K, k):
  """forward / grads derive (taps, pad) from k; the tap entries take them as given: the model's pad0 is model_pad0."""
  x, w, _, bias, res, dy = _small((2, 3, 4, 4, 5, K, 1, 0), seed=2)
  kf, pad = ur.taps_pad(k, K, gain=1.5)
  assert pad[0] == uc.model_pad0(K, kf.shape[0]) and pad == ur.pad_of(pad[0], kf.shape[0], K)
  a, b = ur.forward(x, w, k, 1.5, bias, res, 1.25), ur.forward_taps(x, w, kf, pad[0], bias, res, 1.25)
  assert all((p - q).abs().max() <= 1e-12 * float(q.abs().max()) for p, q in zip(a, b))
  a, b = ur.grads(x, w, dy, k, 1.5), ur.grads_taps(x, w, dy, kf, pad[0])
  assert all((p - q).abs().max() <= 1e-12 * float(q.abs().max()) for p, q in zip(a, b))


# ---- the bound -----------------------------------------------------------------------------------------------------------
def _round11(t):
  """t rounded to 11 significant bits (what a half-precision operand keeps)."""
  bits = t.contiguous().view(torch.int32)
  return ((bits + 0x1000) & ~0x1FFF).view(torch.float32)


def _worst(delta, bnd):
  return float((delta.abs() / bnd).max())


def _mutants(c, t, want, bnd):
  """name -> the worst |mutant - reference| / bound over the output the mutant changes.  Everything here is linear in the
  operand that is changed, so a mutant's difference is the reference of the changed part alone."""
  d = {k: (None if v is None else v.double()) for k, v in t.items()}
  x, w, kf, dy, u = d['x'], d['w'], d['fir'], d['dy'], want['u']
  K, KT, H, W = c.K, c.KT, c.H, c.W
  UH, UW = 2 * H - 2 + K, 2 * W - 2 + K
  pad = ur.pad_of(c.pad0, KT, K)
  m = {}
  y0, du0 = ur.fir(u, kf, pad), want['du']
  firs = {'pad0 + 1': (kf, c.pad0 + 1), 'pad0 - 1': (kf, c.pad0 - 1)}
  if KT > 1 and c.taps == 'randn':                 # the model's symmetric taps cannot tell: the reason the others are randn
    firs.update({'flip': (torch.flip(kf, [0, 1]), c.pad0), 'transposed': (kf.t().contiguous(), c.pad0)})
  for name, (k2, p0) in firs.items():
    m[f'forward FIR {name}'] = _worst((ur.fir(u, k2, ur.pad_of(p0, KT, K)) - y0) / c.div, bnd['y'])
    m[f'adjoint FIR {name}'] = _worst(ur.fir_adjoint(dy, k2, ur.pad_of(p0, KT, K), UH, UW) - du0, bnd['du'])
  # one weight dropped: the last output and input channel (the tile tails), the largest of their taps (a randn value may
  # happen to be next to nothing, and then its loss is no error)
  co, ci = c.Cout - 1, c.Cin - 1
  kh, kw = divmod(int(w[co, ci].abs().argmax()), K)
  w1 = torch.zeros(1, 1, K, K, dtype=torch.float64)
  w1[0, 0, kh, kw] = w[co, ci, kh, kw]
  m['a weight dropped (y)'] = _worst(ur.forward_taps(x[:, ci:ci + 1], w1, kf, c.pad0)[0] / c.div, bnd['y'][:, co:co + 1])
  m['a weight dropped (dx)'] = _worst(c.a_dx[0] * ur.gather(x[:, ci:ci + 1], w1, du0[:, co:co + 1])[0], bnd['dx_b0'][:, ci:ci + 1])
  # one input pixel dropped: the last image and channel, the largest pixel of that plane.  In the weight gradient it is one
  # term of n = N H W under a bound of n 2^-24 B: it can only show while n^2 2^-24 is small, so only the short sums are asked
  n = c.N - 1
  i, j = divmod(int(x[n, ci].abs().argmax()), W)
  x1 = torch.zeros(1, 1, H, W, dtype=torch.float64)
  x1[0, 0, i, j] = x[n, ci, i, j]
  m['a pixel dropped (y)'] = _worst(ur.forward_taps(x1, w[:, ci:ci + 1], kf, c.pad0)[0] / c.div, bnd['y'][n:n + 1])
  if c.N * H * W <= PIXEL_DW_MAX:
    m['a pixel dropped (dw)'] = _worst(c.a_dw[0] * ur.gather(x1, w[:, ci:ci + 1], du0[n:n + 1])[1], bnd['dw_du'][:, ci:ci + 1])
  # the last slab of the weight gradient dropped (or, with the other sign, doubled)
  T, splits, kps = uc.wg_plan(c)
  if splits > 1:
    k0 = (splits - 1) * kps
    n0 = k0 // (H * W)
    pix = torch.arange(n0 * H * W, c.N * H * W).view(c.N - n0, 1, H, W)      # the GEMM's k index of every pixel
    xs = x[n0:] * (pix >= k0)
    m['a slab dropped or doubled (dw)'] = _worst(c.a_dw[0] * ur.gather(xs, w, du0[n0:])[1], bnd['dw_du'])
  # a parity of the forward reading its taps shifted by one: (s, t) -> the other tap of that parity
  if K == 3 and c.N * c.Cin * c.Cout * H * W <= 6e7:
    for name, sl in (('(0, 0)', (slice(0, 3, 2), slice(0, 3, 2))), ('(0, 1)', (slice(0, 3, 2), slice(1, 2))), ('(1, 0)', (slice(1, 2), slice(0, 3, 2)))):
      wm = torch.zeros_like(w)
      part = w[:, :, sl[0], sl[1]]
      wm[:, :, sl[0], sl[1]] = torch.flip(part, [2, 3]) - part
      m[f'parity {name} taps shifted (y)'] = _worst(ur.forward_taps(x, wm, kf, c.pad0)[0] / c.div, bnd['y'])
  # 11-bit operands in the smallest image of a scaled batch: only where the contraction is short
  if c.scaled:
    n = uc.smallest_image(c.name)
    if c.Cin <= uc.SHORT:
      dxn = (_round11(t['x'][n:n + 1]) - t['x'][n:n + 1]).double()
      m['11-bit x in the smallest image (y)'] = _worst(ur.forward_taps(dxn, w, kf, c.pad0)[0] / c.div, bnd['y'][n:n + 1])
    if c.Cout <= uc.SHORT:
      ddy = (_round11(t['dy'][n:n + 1]) - t['dy'][n:n + 1]).double()
      ddu = ur.fir_adjoint(ddy, kf, pad, UH, UW)
      m['11-bit dy in the smallest image (dx)'] = _worst(c.a_dx[0] * ur.gather(x[n:n + 1], w, ddu)[0], bnd['dx_b0'][n:n + 1])
  return m


@pytest.mark.parametrize('name', uc.IDS)
def test_plain_fp32_is_inside_and_every_mutant_outside_the_bound(name):
  """The condition on the inputs -- the reference evaluated in float32 torch on the CPU stays within the bound, on every
  element of every output of every case -- and the reach of the bound: each mutant is at least 5 bounds away at its worst
  element."""
  c, t = uc.BY_NAME[name], uc.inputs(name)
  want, mag = uc.reference(name)
  bnd = uc.bounds(c, mag)
  got = uc.evaluate(c, t, torch.float32)
  for out in uc.OUTPUTS:
    assert got[out].dtype == torch.float32
    uc.check(c, out, got[out], want[out], bnd[out])
  uc.check_sums(c, 'dw_du', got['dw_du'], c.a_dw[0], want, mag)
  uc.check_sums(c, 'dw_dy', got['dw_dy'], c.a_dw[1], want, mag)
  mutants = _mutants(c, t, want, bnd)
  for what, r in mutants.items():
    print(f'  {name} mutant {what}: {r:.3g} bounds')
  weak = {what: r for what, r in mutants.items() if not r >= MUTANT_FACTOR}
  assert not weak, (name, weak)


def test_every_mutant_kind_is_met_by_some_case():
  kinds = set()
  for c in uc.CASES:
    T, splits, kps = uc.wg_plan(c)
    kinds |= {'fir'} | ({'flip'} if c.KT > 1 else set()) | ({'slab'} if splits > 1 else set())
    kinds |= {'parity'} if c.K == 3 and c.N * c.Cin * c.Cout * c.H * c.W <= 6e7 else set()
    kinds |= {'11-bit y'} if c.scaled and c.Cin <= uc.SHORT else set()
    kinds |= {'11-bit dx'} if c.scaled and c.Cout <= uc.SHORT else set()
    kinds |= {'pixel dw'} if c.N * c.H * c.W <= PIXEL_DW_MAX else set()
  assert kinds == {'fir', 'flip', 'slab', 'parity', '11-bit y', '11-bit dx', 'pixel dw'}
