"""The entries of include/stk_guided.h (csrc/guided.hip) through ctypes, on the device: the per-sample order statistic
against a full sort, bit for bit; the thresholded solver step against its fp32 restatement (d_raw, q: bit for bit) and against
float64 with the forward-error form of tests/test_gpu_dpm_solver.py (x_out, d_out: gamma_k times the expression on absolute
values, k one more than the plain update's for the division by s, the scale s entering the reference as the fp32 value the
kernel selected); the guidance rescale against the float64 restatement computed from the fp32 g (3 u |want|: f rounded to
fp32, the product, one for the float64 variance).  Every output starts as NaN (q as a sentinel), every call is made twice and
the two results compared bit for bit."""
import numpy as np
import pytest
import torch

import _guided_ref as G
from _stream_util import case_id, place, stream as _stream, within

pytestmark = pytest.mark.gpu

NAN = float('nan')
EINVAL, EUNSUPPORTED = -1, -3
f32 = lambda v: float(np.float32(v))
ROW = tuple(f32(v) for v in (1.3, 0.7, 0.45, 0.8, 0.35))          # (cx, cs, g, A, B): a second-order step


def _ws(lib, B, n, dev):
  nbytes = int(lib.guided_ws_bytes(B, n))
  assert nbytes >= B * 16384
  return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev), nbytes


def _select(lib, v, B, n, rank, ws, nbytes, first_level_done=0):
  """q of one call, as a numpy float32 vector; q starts as a sentinel."""
  q = torch.full((B,), -7.0, dtype=torch.float32, device=v.device)
  lib.abs_select_f32(v.data_ptr(), B, n, rank, q.data_ptr(), ws.data_ptr(), nbytes, first_level_done, _stream())
  return q.cpu().numpy()


# ---- selection ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,shifted', G.SHAPES, ids=case_id)
def test_select_is_the_sorted_element(hip_lib, shape, shifted):
  dev = torch.device('cuda:0')
  B, n = shape
  ws, nbytes = _ws(hip_lib, B, n, dev)
  for kind in G.CONTENTS:
    v = G.content(kind, B, n)
    vd = place(v, dev, shifted)
    assert (vd.data_ptr() % 16 == 4) == shifted
    for rank in G.ranks(n):
      want = G.select(v, rank)
      got = _select(hip_lib, vd, B, n, rank, ws, nbytes)
      again = _select(hip_lib, vd, B, n, rank, ws, nbytes)
      what = f'select {shape} shifted={shifted} {kind} rank {rank}'
      assert np.array_equal(G.bits(got), G.bits(again)), what + ': two calls differ'
      bad = np.nonzero(G.bits(got) != G.bits(want))[0]
      assert bad.size == 0, f'{what}: row {bad[0]} got {got[bad[0]]!r} ({G.bits(got)[bad[0]]:#x}), want {want[bad[0]]!r}'
      if kind == 'one-nan':
        assert np.isnan(got[0]) == (rank == n - 1) and not np.isnan(got[1:]).any()
    assert np.array_equal(G.bits(vd.cpu().numpy()), G.bits(v)), 'the operand was written'


def test_select_return_codes_and_nothing_written(hip_lib):
  dev = torch.device('cuda:0')
  raw = hip_lib.abs_select_f32.raw
  B, n = 2, 192
  v = torch.randn(B, n, device=dev)
  q = torch.full((B,), 7.0, device=dev)
  ws, nbytes = _ws(hip_lib, B, n, dev)
  ptr = lambda t: None if t is None else t.data_ptr()

  def rc(v=v, B=B, n=n, rank=5, no_q=False, no_ws=False, nbytes=nbytes, done=0, ws_off=0):
    code = raw(ptr(v), B, n, rank, None if no_q else q.data_ptr(), None if no_ws else ws.data_ptr() + ws_off, nbytes, done, _stream())
    torch.cuda.synchronize()
    assert bool((q == 7.0).all()) and bool((ws == 0xA5).all()), 'a refused call wrote'
    return code

  assert rc(v=None) == EINVAL and rc(no_q=True) == EINVAL and rc(no_ws=True) == EINVAL
  assert rc(B=0) == EINVAL and rc(B=-1) == EINVAL and rc(n=0) == EINVAL and rc(n=-3) == EINVAL
  assert rc(rank=-1) == EINVAL and rc(rank=n) == EINVAL and rc(rank=n + 7) == EINVAL
  assert rc(nbytes=nbytes - 1) == EINVAL and rc(nbytes=0) == EINVAL
  assert rc(ws_off=4, nbytes=nbytes - 4) == EINVAL                      # a misaligned workspace
  assert rc(done=2) == EINVAL and rc(done=-1) == EINVAL
  assert rc(B=2, n=2 ** 30) == EUNSUPPORTED and rc(B=1, n=2 ** 31) == EUNSUPPORTED and rc(B=2 ** 16, n=2 ** 15) == EUNSUPPORTED
  assert int(hip_lib.guided_ws_bytes(0, 4)) == EINVAL and int(hip_lib.guided_ws_bytes(4, 0)) == EINVAL
  assert int(hip_lib.guided_ws_bytes(2, 2 ** 30)) == EUNSUPPORTED
  assert int(hip_lib.guided_ws_bytes(1, 3 * 256 * 256)) > 16384          # one row, many blocks: the rescale's partials
  # the accepted edge forms run, and the checked binding raises the package's error
  assert raw(ptr(v), B, n, 0, torch.empty_like(q).data_ptr(), ws.clone().data_ptr(), nbytes, 0, _stream()) == 0
  with pytest.raises(RuntimeError, match='stk_abs_select_f32 failed'):
    hip_lib.abs_select_f32(v.data_ptr(), B, n, n, q.data_ptr(), ws.data_ptr(), nbytes, 0, _stream())
  torch.cuda.synchronize()


# ---- the thresholded step ---------------------------------------------------------------------------------------------------
def _predict(lib, x, s, row, d_raw, B, n, ws, nbytes):
  lib.dpm_predict_f32(x.data_ptr(), s.data_ptr(), row[0], row[1], d_raw.data_ptr(), B, n, ws.data_ptr(), nbytes, _stream())


def _apply(lib, x, d_raw, d_prev, q, floor, row, x_out, d_out, B, n):
  ptr = lambda t: None if t is None else t.data_ptr()
  lib.dpm_threshold_update_f32(ptr(x), d_raw.data_ptr(), ptr(d_prev), q.data_ptr(), floor, row[2], row[3], row[4], ptr(x_out),
                               ptr(d_out), B, n, _stream())


@pytest.fixture(scope='module')
def step_operands():
  """x, score, d_prev per shape as float32 numpy [B, n]: drawn once."""
  out = {}
  for shape in sorted({s for s, _ in G.SHAPES}):
    rng = np.random.RandomState(sum(shape))
    out[shape] = tuple((rng.standard_normal(shape) * scale).astype(np.float32) for scale in (1.5, 2.0, 1.0))
  return out


@pytest.mark.parametrize('shape,shifted', G.SHAPES, ids=case_id)
def test_thresholded_step(hip_lib, step_operands, shape, shifted):
  dev = torch.device('cuda:0')
  B, n = shape
  x, s, p = step_operands[shape]
  xd, sd, pd = (place(t, dev, shifted) for t in (x, s, p))
  ws, nbytes = _ws(hip_lib, B, n, dev)
  rank = G.rank_of(0.9, n)
  # predict: d_raw bit for bit, twice
  want_raw = G.predict32(x, s, ROW[0], ROW[1])
  raws = []
  for _ in range(2):
    d_raw = place(np.full(shape, NAN, dtype=np.float32), dev, shifted)
    _predict(hip_lib, xd, sd, ROW, d_raw, B, n, ws, nbytes)
    raws.append(d_raw)
  assert torch.equal(raws[0], raws[1])
  assert np.array_equal(G.bits(raws[1].cpu().numpy()), G.bits(want_raw)), f'{shape}: d_raw differs from the fp32 restatement'
  d_raw = raws[1]
  # q from the histogram the predict pass left, and from a selection of its own: the sorted restatement of that d_raw
  want_q = G.select(want_raw, rank)
  q_fused = _select(hip_lib, d_raw, B, n, rank, ws, nbytes, first_level_done=1)
  # ... which leaves the first level in place: repeated on the same prediction, with another rank and with the same
  for again in (0, n - 1, rank):
    q_again = _select(hip_lib, d_raw, B, n, again, ws, nbytes, first_level_done=1)
    assert np.array_equal(G.bits(q_again), G.bits(G.select(want_raw, again))), f'{shape}: a repeated selection, rank {again}'
  q_own = _select(hip_lib, d_raw, B, n, rank, ws, nbytes)
  assert np.array_equal(G.bits(q_fused), G.bits(want_q)), f'{shape}: q with the first level taken in the predict pass'
  assert np.array_equal(G.bits(q_own), G.bits(want_q))
  qd = torch.from_numpy(want_q).to(dev)
  x64, s64, p64 = (t.astype(np.float64) for t in (x, s, p))
  med = float(np.median(want_q))
  worst_x = worst_d = 0.0
  for floor in (f32(med * 0.5) or 0.25, f32(med * 2.0) or 0.25):       # below and above (most of) q
    scale = G.scale_of(want_q, floor)
    assert scale.dtype == np.float32
    for use_prev in (True, False):
      for use_dout in (True, False):
        row = ROW if use_prev else ROW[:2] + (0.,) + ROW[3:]
        want_x, want_d, b_x, b_d = G.step64(x64, s64, p64 if use_prev else None, row, scale.astype(np.float64))
        outs = []
        for _ in range(2):
          x_out = place(np.full(shape, NAN, dtype=np.float32), dev, shifted)
          d_out = place(np.full(shape, NAN, dtype=np.float32), dev, shifted) if use_dout else None
          _apply(hip_lib, xd, d_raw, pd if use_prev else None, qd, floor, row, x_out, d_out, B, n)
          outs.append((x_out, d_out))
        what = f'threshold_update {shape} shifted={shifted} floor={floor} d_prev={use_prev} d_out={use_dout}'
        assert torch.equal(outs[0][0], outs[1][0]), what + ': two calls differ'
        x_out, d_out = outs[1]
        worst_x = max(worst_x, within(x_out.view(B, n), want_x, b_x, G.K_X, what + ' x_out'))
        if use_dout:
          assert torch.equal(outs[0][1], outs[1][1])
          worst_d = max(worst_d, within(d_out.view(B, n), want_d, b_d, G.K_D, what + ' d_out'))
          assert float(d_out.abs().max()) <= 1.0, what + ': |d| above 1'
          # d is the fp32 restatement bit for bit: one clamp, one division
          assert np.array_equal(G.bits(d_out.cpu().numpy()), G.bits(G.threshold(want_raw, scale))), what
        # state and history kept in place: bit-identical to the separate-buffer form
        xa, pa = place(x, dev, shifted), place(p, dev, shifted)
        _apply(hip_lib, xa, d_raw, pa if use_prev else None, qd, floor, row, xa, pa if (use_prev and use_dout) else d_out, B, n)
        assert torch.equal(xa, x_out), what + ': x_out = x differs from the separate-buffer form'
        if use_prev and use_dout:
          assert torch.equal(pa, d_out), what + ': d_out = d_prev differs from the separate-buffer form'
    # the thresholding alone: x and x_out NULL
    only = place(np.full(shape, NAN, dtype=np.float32), dev, shifted)
    _apply(hip_lib, None, d_raw, None, qd, floor, ROW[:2] + (0.,) + ROW[3:], None, only, B, n)
    assert np.array_equal(G.bits(only.cpu().numpy()), G.bits(G.threshold(want_raw, scale)))
  assert bool((want_q > f32(med * 0.5)).any()) and bool((want_q < f32(med * 2.0)).any()), 'floor on one side only'
  assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(sd.cpu().numpy(), s) and np.array_equal(pd.cpu().numpy(), p)
  print(f'thresholded step {shape} shifted={shifted}: worst x_out {worst_x:.2f} u B (bound {G.K_X}), worst d_out {worst_d:.2f} u B '
        f'(bound {G.K_D})')


def test_thresholded_step_shows_a_nan_row(hip_lib):
  """A NaN among the scores of row 0 at the top rank: q[0], s and the whole row of d and x_out are NaN; row 1 is untouched."""
  dev = torch.device('cuda:0')
  B, n = 2, 192
  rng = np.random.RandomState(3)
  x, s = ((rng.standard_normal((B, n)) * 1.5).astype(np.float32) for _ in range(2))
  s[0, 17] = np.float32('nan')
  clean = s.copy()
  clean[0, 17] = 0.5
  ws, nbytes = _ws(hip_lib, B, n, dev)
  res = {}
  for name, score in (('nan', s), ('clean', clean)):
    xd, sd = place(x, dev), place(score, dev)
    d_raw, x_out, d_out = (torch.full((B, n), NAN, device=dev) for _ in range(3))
    _predict(hip_lib, xd, sd, ROW, d_raw, B, n, ws, nbytes)
    q = torch.from_numpy(_select(hip_lib, d_raw, B, n, n - 1, ws, nbytes, first_level_done=1)).to(dev)
    _apply(hip_lib, xd, d_raw, None, q, 0.5, ROW[:2] + (0.,) + ROW[3:], x_out, d_out, B, n)
    res[name] = (q.cpu(), x_out.cpu(), d_out.cpu())
  q, x_out, d_out = res['nan']
  assert bool(torch.isnan(q[0])) and bool(torch.isnan(x_out[0]).all()) and bool(torch.isnan(d_out[0]).all())
  assert torch.equal(q[1], res['clean'][0][1]) and torch.equal(x_out[1], res['clean'][1][1]) and torch.equal(d_out[1], res['clean'][2][1])
  assert bool(torch.isfinite(res['clean'][1]).all())


def test_step_return_codes_and_nothing_written(hip_lib):
  dev = torch.device('cuda:0')
  B, n = 2, 192
  x, s, p, d_raw = (torch.randn(B, n, device=dev) for _ in range(4))
  q = torch.ones(B, device=dev)
  x_out, d_out, raw_out = (torch.full((B, n), 7.0, device=dev) for _ in range(3))
  ws, nbytes = _ws(hip_lib, B, n, dev)
  ptr = lambda t: None if t is None else t.data_ptr()
  INF = float('inf')

  def untouched():
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (x_out, d_out, raw_out)) and bool((ws == 0xA5).all()), 'a refused call wrote'

  def predict(x=x, s=s, out=raw_out, B=B, n=n, no_ws=False, nbytes=nbytes, ws_off=0):
    code = hip_lib.dpm_predict_f32.raw(ptr(x), ptr(s), 1.3, 0.7, ptr(out), B, n, None if no_ws else ws.data_ptr() + ws_off,
                                       nbytes, _stream())
    untouched()
    return code

  assert predict(x=None) == EINVAL and predict(s=None) == EINVAL and predict(out=None) == EINVAL and predict(no_ws=True) == EINVAL
  assert predict(B=0) == EINVAL and predict(n=0) == EINVAL and predict(n=-4) == EINVAL
  assert predict(nbytes=nbytes - 1) == EINVAL and predict(ws_off=8, nbytes=nbytes - 8) == EINVAL
  assert predict(B=2, n=2 ** 30) == EUNSUPPORTED and predict(B=1, n=2 ** 31) == EUNSUPPORTED

  def update(x=x, d_raw=d_raw, p=p, q=q, floor=1.0, g=0.45, x_out=x_out, d_out=d_out, B=B, n=n):
    code = hip_lib.dpm_threshold_update_f32.raw(ptr(x), ptr(d_raw), ptr(p), ptr(q), floor, g, 0.8, 0.35, ptr(x_out), ptr(d_out), B,
                                                n, _stream())
    untouched()
    return code

  assert update(d_raw=None) == EINVAL and update(q=None) == EINVAL
  assert update(x=None) == EINVAL and update(x_out=None) == EINVAL            # exactly one of the pair
  assert update(x=None, x_out=None, d_out=None) == EINVAL                      # nothing to write
  assert update(p=None, g=0.45) == EINVAL and update(p=None, g=-0.1) == EINVAL
  assert update(floor=0.) == EINVAL and update(floor=-1.) == EINVAL and update(floor=NAN) == EINVAL and update(floor=INF) == EINVAL
  assert update(B=0) == EINVAL and update(n=0) == EINVAL
  assert update(B=2, n=2 ** 30) == EUNSUPPORTED and update(B=1, n=2 ** 31) == EUNSUPPORTED
  assert update(p=None, g=0., x_out=torch.empty_like(x), d_out=None) == 0
  with pytest.raises(RuntimeError, match='stk_dpm_threshold_update_f32 failed'):
    hip_lib.dpm_threshold_update_f32(x.data_ptr(), d_raw.data_ptr(), None, q.data_ptr(), 1.0, 0.45, 0.8, 0.35, x_out.data_ptr(), None,
                                     B, n, _stream())
  torch.cuda.synchronize()


# ---- guidance rescale ---------------------------------------------------------------------------------------------------------
def _rescale(lib, c, u, w, phi, out, B, n, ws, nbytes):
  lib.cfg_rescale_f32(c.data_ptr(), u.data_ptr(), w, phi, out.data_ptr(), B, n, ws.data_ptr(), nbytes, _stream())


@pytest.mark.parametrize('shape,shifted', G.SHAPES, ids=case_id)
def test_rescale(hip_lib, shape, shifted):
  dev = torch.device('cuda:0')
  B, n = shape
  c, u = G.rescale_operands(B, n, constant_row=B - 1 if B > 1 else None)
  cd, ud = place(c, dev, shifted), place(u, dev, shifted)
  ws, nbytes = _ws(hip_lib, B, n, dev)

  def run(w, phi):
    outs = []
    for _ in range(2):
      o = place(np.full(shape, NAN, dtype=np.float32), dev, shifted)
      _rescale(hip_lib, cd, ud, w, phi, o, B, n, ws, nbytes)
      outs.append(o)
    assert torch.equal(outs[0], outs[1]), f'rescale {shape} w={w} phi={phi}: two calls differ'
    return outs[1]

  w, phi = f32(2.0), f32(0.7)
  # phi = 0: the bits of stk_cfg_combine_f32 (and of the fp32 restatement)
  comb = place(np.full(shape, NAN, dtype=np.float32), dev, shifted)
  hip_lib.cfg_combine_f32(cd.data_ptr(), ud.data_ptr(), w, comb.data_ptr(), B * n, _stream())
  assert torch.equal(run(w, 0.0), comb), f'rescale {shape}: phi = 0 is not stk_cfg_combine_f32'
  assert np.array_equal(G.bits(comb.cpu().numpy()), G.bits(G.combine32(c, u, w)))
  # w = 0: f = 1 exactly
  assert torch.equal(run(0.0, phi), cd), f'rescale {shape}: w = 0 does not return cond'
  worst = 0.0
  for w_, phi_ in ((w, phi), (w, 1.0), (f32(-0.5), f32(0.3)), (f32(7.5), phi)):
    want, g32, f = G.rescale64(c, u, w_, phi_)
    got = run(w_, phi_)
    what = f'rescale {shape} shifted={shifted} w={w_} phi={phi_}'
    worst = max(worst, within(got.view(B, n), want, np.abs(want), G.K_RESCALE, what))
    if B > 1:                                        # the constant row: sigma_g = 0, f = 1
      assert f[B - 1] == 1.0 and np.array_equal(G.bits(got.view(B, n)[B - 1].cpu().numpy()), G.bits(g32[B - 1])), what
  # out may be cond or uncond
  want = run(w, phi)
  for alias in ('cond', 'uncond'):
    ca, ua = place(c, dev, shifted), place(u, dev, shifted)
    o = ca if alias == 'cond' else ua
    _rescale(hip_lib, ca, ua, w, phi, o, B, n, ws, nbytes)
    assert torch.equal(o, want), f'rescale {shape}: out = {alias} differs from the separate-buffer form'
  assert np.array_equal(cd.cpu().numpy(), c) and np.array_equal(ud.cpu().numpy(), u), 'an operand was written'
  print(f'rescale {shape} shifted={shifted}: worst {worst:.2f} u |want| (bound {G.K_RESCALE})')


def test_rescale_return_codes_and_nothing_written(hip_lib):
  dev = torch.device('cuda:0')
  B, n = 2, 192
  c, u = (torch.randn(B, n, device=dev) for _ in range(2))
  out = torch.full((B, n), 7.0, device=dev)
  ws, nbytes = _ws(hip_lib, B, n, dev)
  ptr = lambda t: None if t is None else t.data_ptr()
  INF = float('inf')

  def rc(c=c, u=u, w=2.0, phi=0.7, no_out=False, B=B, n=n, no_ws=False, nbytes=nbytes, ws_off=0):
    code = hip_lib.cfg_rescale_f32.raw(ptr(c), ptr(u), w, phi, None if no_out else out.data_ptr(), B, n, None if no_ws else ws.data_ptr() + ws_off, nbytes,
                                       _stream())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0xA5).all()), 'a refused call wrote'
    return code

  assert rc(c=None) == EINVAL and rc(u=None) == EINVAL and rc(no_out=True) == EINVAL and rc(no_ws=True) == EINVAL
  assert rc(B=0) == EINVAL and rc(n=0) == EINVAL and rc(n=-4) == EINVAL
  assert rc(w=NAN) == EINVAL and rc(w=INF) == EINVAL
  assert rc(phi=-0.01) == EINVAL and rc(phi=1.01) == EINVAL and rc(phi=NAN) == EINVAL and rc(phi=INF) == EINVAL
  assert rc(nbytes=nbytes - 1) == EINVAL and rc(ws_off=8, nbytes=nbytes - 8) == EINVAL
  assert rc(B=2, n=2 ** 30) == EUNSUPPORTED and rc(B=1, n=2 ** 31) == EUNSUPPORTED
  with pytest.raises(RuntimeError, match='stk_cfg_rescale_f32 failed'):
    hip_lib.cfg_rescale_f32(c.data_ptr(), u.data_ptr(), 2.0, 1.5, out.data_ptr(), B, n, ws.data_ptr(), nbytes, _stream())
  # the ends of the range of phi are accepted
  for phi in (0.0, 1.0):
    assert hip_lib.cfg_rescale_f32.raw(ptr(c), ptr(u), 2.0, phi, torch.empty_like(c).data_ptr(), B, n, ws.data_ptr(), nbytes, _stream()) == 0
  torch.cuda.synchronize()
