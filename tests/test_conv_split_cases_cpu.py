"""The case table, the two instruments and the numpy model of the split-convolution tests, without a GPU
(tests/_conv_split_cases.py, tests/_conv_split_ref.py; the GPU half is tests/test_gpu_conv_split_forms.py).

  - the table reaches every form, direction and family by the restated plan, and the shapes that never ran before:
    short last splits, more than 9 images in a tile with temb, dead rows, one chunk per tap, two sources;
  - instrument A: the exact operands split as claimed, every partial sum fits 24 bits (exactness() <= 2^24),
    three_term + sum lo lo == the float64 product bit for bit, and the float32 model equals three_term bit for bit in
    the kernels' order of accumulation and in a shuffled one;
  - instrument B: the float64 reference is F.conv2d / autograd; the model stays within HALF of every bound on every other
    case; in the faint cases the floor is more than half of the faint image's bound and the model's error there exceeds
    the rounding part alone;
  - every mutant of the model is caught on the case named for it: off by at least one bit on an exact case, or at least
    5 bounds out on a bound case;
  - the table that says why a derived bound alone is not enough (K = 32, 288, 864) is reproduced and printed.
The model depends on the operands, not on the entry that runs them: cases that differ in the entry alone are run once.
Ratios are printed per case with -s."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_split_cases as cc
import _conv_split_ref as cr


def _unique():
  seen, out = set(), []
  for n, c in cc.BY_NAME.items():
    if (c.row, c.d, c.fam) not in seen:
      seen.add((c.row, c.d, c.fam))
      out.append(n)
  return out


UNIQUE = _unique()
EXACT = [n for n in UNIQUE if cc.BY_NAME[n].fam in cc.EXACT_FAMILIES]
BOUND = [n for n in UNIQUE if cc.BY_NAME[n].fam not in cc.EXACT_FAMILIES]


def test_table_reaches_every_form_direction_and_family():
  reached = set()
  for c in cc.CASES:
    r = cc.BY_ROW[c.row]
    got = cc.plan(r, c.entry)
    assert got is not None, c
    form, splits = got
    if c.entry == 'pl':
      assert form == r.form, (c, form)
    else:
      assert form == ('ks' if r.form == 'ks' else ('g9' if r.taps == 9 else 'g1')), (c, form)
    assert r.form != 'ks' or splits == cc.EXPECTED_SPLITS[r.name], (c, splits)
    reached.add((cc.form_key(r), c.d, c.entry, c.fam))
  for form in cc.FORMS:
    for d in 'fd':
      for fam in cc.FAMILIES:
        assert (form, d, 'pl', fam) in reached, (form, d, fam)
  for form in ('g9', 'g1', 'ks9', 'ks1'):                  # the f32-operand entries take the g9, g1 and both ks rows
    for d in 'fd':
      for fam in cc.EXACT_FAMILIES + ('randn',):
        assert (form, d, 'f32', fam) in reached, (form, d, fam)
  rows = cc.BY_ROW
  assert any(len(set(s)) > 1 for s in cc.EXPECTED_SPLITS.values())                        # a short last split, 3x3 and 1x1
  assert cc.EXPECTED_SPLITS['ks_14+13'][-1] % 2 == 1 and cc.EXPECTED_SPLITS['ks_4x13+11'][-1] % 2 == 1
  assert cc.EXPECTED_SPLITS['ks1_7+6'] == (7, 6) and cc.EXPECTED_SPLITS['ks1_6+6'] == (6, 6)
  assert all(128 // (rows[n].H * rows[n].W) > 9 for n in ('g9_3x3', 'g9_2x2'))            # EpFwd's unstaged temb branch
  assert (rows['g9_3x3'].N * 9) % 128 != 0                                                # ... with a ragged last tile
  assert rows['h16_dead'].M == 96 and rows['h16_ragged'].M % 128 == 8 and rows['h16'].Kc == 32
  assert {(rows[n].S1, rows[n].Kc - rows[n].S1) for n in ('g9_src2', 'ks_src2')} == {(32, 64), (96, 32)}
  assert 'g9_src2_fwd_f32_src2x1e4' in cc.BY_NAME
  assert any(rows[c.row].layout == 1 and rows[c.row].form == 'g1' for c in cc.CASES)


@pytest.mark.parametrize('name', EXACT)
def test_exact_operands_and_model_bit_for_bit(name):
  c = cc.BY_NAME[name]
  r = cc.BY_ROW[c.row]
  t, p = cc.inputs(name), cc.problem_of(name)
  hmax = 2 if r.Kc * r.taps <= 864 else 1
  for k in ('a', 'w'):
    assert cr.is_exact_split(t[k], hmax), k
    flat = np.abs(t[k]).reshape(-1)
    assert flat.max() == 2.0
    assert np.abs(t[k][np.abs(t[k]) != 2.0]).max() <= (2.0 if hmax == 2 else 1.0 + cr.GRANULE)
  idx, pix = cc.model_subset(name)
  worst = float(cr.exactness(p, idx).max())
  # ... and for every image, whatever the draw: K hmax^2 (1 + 2^-11) plus the one 2 and the addends
  top = (r.Kc * r.taps * hmax * hmax + 4) * (1 + 2.0 ** -11) + (8 if c.fam == 'exact-ep' else 0)
  assert worst <= 2.0 ** 24 and top <= 4096.0, (worst, top)
  tt = cr.three_term(p, idx)
  ref = cr.reference(p, idx)
  assert np.array_equal(tt['out'] + tt['lolo'], ref), 'three_term + sum lo lo is not the float64 product'
  want = cr.at(tt['out'], pix)
  for order in (None, 7):
    got = cr.model(p, idx, pix, order=order)
    assert np.array_equal(got.astype(np.float64), want), f'{name}: the model (order {order}) is not three_term'
  print(f'  {name}: {worst / 2.0 ** 24:.3f} of 24 bits, sum lo lo up to {np.abs(tt["lolo"]).max() * 2.0 ** 24:.0f} x 2^-24')


@pytest.mark.parametrize('name', ['g9_12x20_fwd_pl_randn', 'h16_ragged_dgrad_pl_randn', 'ks1_nin_fwd_pl_randn', 'ks1_nin_dgrad_pl_randn',
                                  'g9_src2_fwd_f32_randn', 'ks_14+13_dgrad_pl_exact-ep'])
def test_reference_is_conv2d_and_autograd(name):
  c = cc.BY_NAME[name]
  r = cc.BY_ROW[c.row]
  t, p = cc.inputs(name), cc.problem_of(name)
  K = 3 if r.taps == 9 else 1
  C1, C2, Cout = cc.layer(r, c.d)
  idx = [0, r.N - 1]
  w = torch.from_numpy(t['w']).double()
  w = w.t().reshape(Cout, C1 + C2, 1, 1) if r.layout == 1 else w
  a = torch.from_numpy(t['a'][idx]).double()
  if c.d == 'f':
    want = F.conv2d(a, w, padding=K // 2)
    want = (want + torch.from_numpy(t['bias']).double()[None, :, None, None] + torch.from_numpy(t['temb'][idx, 8:8 + r.M]).double()[:, :, None, None]
            + torch.from_numpy(t['res'][idx]).double()) / float(np.float32(t['div']))
  else:
    x = torch.zeros(2, C1 + C2, r.H, r.W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, padding=K // 2).backward(a)
    want = x.grad * float(np.float32(t['alpha']))
    for rows, b in ((slice(0, C1), t['beta'][0]), (slice(C1, C1 + C2), t['beta'][1])):
      if b:
        want[:, rows] += float(np.float32(b)) * torch.from_numpy(t['dx0'][idx][:, rows]).double()
  got = cr.reference(p, idx)
  assert np.isfinite(got).all()
  assert np.abs(got - want.numpy()).max() <= 1e-12 * np.abs(want.numpy()).max()


@pytest.mark.parametrize('name', BOUND)
def test_model_within_half_of_every_bound(name):
  c = cc.BY_NAME[name]
  r = cc.BY_ROW[c.row]
  p = cc.problem_of(name)
  idx, pix = cc.model_subset(name)
  pt = cr.parts(p, idx)
  ref, b = cr.at(cr.reference(p, idx, pt), pix), cr.bound(p, idx, pt)
  got = cr.model(p, idx, pix)
  q = cr.ratio(got, ref, cr.at(b['bound'], pix))
  msg = f'  {name}: model err / bound {q.max():.3f}'
  assert q.max() <= 0.5, f'{name}: the model is {q.max():.3g} bounds out'
  if c.fam == 'faint':
    i = idx.index(r.N - 1)
    fl, bu = cr.at(b['F'], pix)[i], cr.SECOND_ORDER * cr.U * cr.at(b['Bu'], pix)[i]
    err = np.abs(got[i].astype(np.float64) - ref[i])
    assert (fl > bu).all(), f'{name}: the floor is not more than half of the faint image\'s bound everywhere'
    assert err.max() > bu[np.unravel_index(err.argmax(), err.shape)], f'{name}: the rounding part alone covers the model'
    msg += f', faint image: floor / rounding part >= {float((fl / bu).min()):.3g}, err / rounding part {float((err / bu).max()):.3g}'
  if c.fam == 'tiny':
    with np.errstate(over='ignore'):
      assert np.float32(cr.pow2_scale_of(np.abs(p.a).max())) * np.float32(cr.pow2_scale_of(np.abs(p.W).max())) == np.inf
    assert np.abs(ref).max() > 2.0 ** -120 and (got != 0).mean() > 0.99           # normal fp32 results, not zeros
  print(msg)


# mutant -> the case expected to catch it
CAUGHT_BY = {
  'hi lo dropped': 'h16_fwd_pl_exact',
  'lo hi dropped': 'h16_two_dgrad_pl_exact',
  'lo at half weight': 'g1_fwd_pl_exact',
  'lo at double weight': 'ks1_7+6_dgrad_pl_exact',
  'lo lo added': 'h32_fwd_pl_exact',
  'tap dropped': 'g9_8x8_fwd_pl_exact',
  'taps flipped': 'g9_8x8_dgrad_pl_exact',
  'taps transposed': 'h64_fwd_pl_exact',
  'right border not padded': 'g9_12x20_fwd_pl_randn',
  'slab dropped': 'ks_even_fwd_pl_exact',
  'slab summed twice': 'ks1_6+6_dgrad_pl_exact-ep',
  'short split truncated': 'ks_14+13_fwd_pl_exact',
  'second source with beta1': 'h16_two_dgrad_pl_randn',
  'dead rows written': 'h16_dead_fwd_pl_exact-ep',
  'temb of the tile\'s first image': 'g9_3x3_fwd_pl_exact-ep',
  'bias before unscale': 'g1_fwd_pl_randn',
  'out_div on the accumulator only': 'g1_nin_fwd_pl_exact-ep',
  'scale of the first source': 'g9_src2_fwd_f32_src2x1e4',
  'unscale in one division': 'ks_14+13_fwd_pl_tiny',
}


def test_every_mutant_has_a_case():
  assert set(CAUGHT_BY) == set(cr.MUTANTS) and all(n in cc.BY_NAME for n in CAUGHT_BY.values())


@pytest.mark.parametrize('mutant', list(CAUGHT_BY))
def test_mutant_is_caught(mutant):
  name = CAUGHT_BY[mutant]
  c = cc.BY_NAME[name]
  p = cc.problem_of(name)
  idx, pix = cc.model_subset(name)
  got = cr.model(p, idx, pix, mutant=mutant)
  if c.fam in cc.EXACT_FAMILIES:
    want = cr.at(cr.three_term(p, idx)['out'], pix)
    off = ~(got.astype(np.float64) == want)
    print(f'  {mutant}: caught by {name}, {100 * off.mean():.1f} % of the elements differ')
    assert off.any(), f'{mutant}: bit-equal to three_term on {name}'
  else:
    ref, b = cr.at(cr.reference(p, idx), pix), cr.at(cr.bound(p, idx)['bound'], pix)
    q = float(cr.ratio(got, ref, b).max())
    print(f'  {mutant}: caught by {name}, {q:.3g} bounds out')
    assert q >= 5.0, f'{mutant}: at most {q:.3g} bounds out on {name}: the bound would let it pass'


def test_why_a_derived_bound_alone_is_not_enough():
  """randn operands, weights over sqrt K, images spread over 4 decades: the correct product sits far inside the derived
  bound, and at K = 864 so does a product that lost a whole cross term.  Printed for the record.  (The figures that
  motivated the design were 0.027 / 27, 0.004 / 1.06 and 0.002 / 0.20; this sample is 8 images of 32 x 8 x 8 outputs.)"""
  rows = []
  for taps, C in ((1, 32), (9, 32), (9, 96)):
    g = np.random.default_rng(C * taps)
    N, M, H = 8, 32, 8
    a = g.standard_normal((N, C, H, H)).astype(np.float32) * np.logspace(-4, 0, N).astype(np.float32)[:, None, None, None]
    W = (g.standard_normal((M, C, taps)) / np.sqrt(C * taps)).astype(np.float32)
    p = cr.problem(False, a, W, taps)
    ref, b = cr.reference(p).reshape(N, M, -1), cr.bound(p)['bound'].reshape(N, M, -1)
    good = float(cr.ratio(cr.model(p), ref, b).max())
    bad = float(cr.ratio(cr.model(p, mutant='hi lo dropped'), ref, b).max())
    rows.append((C * taps, good, bad))
    print(f'  K = {C * taps:4d}: correct product / bound {good:.4f}, one cross term dropped {bad:.3g} bounds out')
  assert all(good <= 0.5 for _, good, _ in rows)
  assert rows[0][2] >= 5.0, 'K = 32: the bound alone catches the lost cross term'
  assert rows[2][2] < 1.0, 'K = 864: the lost cross term sits inside the bound -- the reason instrument A exists'
