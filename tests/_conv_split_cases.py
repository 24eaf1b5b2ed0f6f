"""The case table of the split-convolution tests, the launch plan restated, and one runner per direction
(tests/test_conv_split_cases_cpu.py without a GPU, tests/test_gpu_conv_split_forms.py on one; reference, bounds and
model: tests/_conv_split_ref.py).

Rows are written in the GEMM view of _conv_split_ref.py: Kc channels are contracted into M output rows.  The forward
case of a row is the layer Cin = Kc -> Cout = M; the data-gradient case is the layer Cin = M <- Cout = Kc, so that both
directions of a row reach the same plan (the data gradient of the forward's layer would have M = Kc rows, which the plan
refuses under 96).  C1 > 0 gives the data gradient two destinations (rows [0, C1) and [C1, M)); S1 > 0 gives the forward
of the f32-operand entry two sources (channels [0, S1) and [S1, Kc)), which planes cannot express.

plan() restates split_plan / halo_ok of csrc/conv.hip and csrc/conv_x2d.h; on the device every case also asserts its
form through the library's own diagnostics (stk_conv2d_pl_ok, _pl_ksplit, _pl_halo, stk_conv2d_variant).

Families.  'exact' and 'exact-ep' (instrument A, every row): exact operands bare, and with the full exact epilogue --
forward: dyadic bias, temb read as a column slice of a wider tensor, res, out_div 2; data gradient: alpha 0.5, beta1 0.5
on a dyadic dx0, and beta2 0 on a NaN-filled dx2 where the row has two destinations.  The other families run under the
bound, on the smallest row of every form and direction (BOUND_ROWS) -- 'randn' on every row:
  randn     the epilogue of tests/test_gpu_contractions.py: bias, temb, res, out_div sqrt 2; alpha 0.5, beta 0.25 (one
            destination) or 0 / 0.75 (two)
  spread    per-image factors over 4 decades          faint   the last image at 2^-30 of the batch maximum
  pow2      maximum exactly 4 (the floor(log2) edge)  tiny    max |a| = 2^-60, max |w| = 2^-50 (sa sw = 2^136: overflows fp32)
  huge      maxima 2^40 and 2^20                      wtiny   a ordinary, max |w| = 2^-100
All but randn run bare (no addends, out_div 1, alpha 1, beta 0 on NaN-filled dx).  All-zero operands stay in
tests/test_gpu_contractions.py.

Departures from the issue text.
  - The N 6144 row of 2 x 2 maps has 24576 pixels, exactly 192 tiles: its last tile is full; the N 2731 row of 3 x 3
    maps (24579 pixels) is the one with the ragged last tile.
  - "32 -> 128, both" is read in the GEMM view (first paragraph): the data gradient's layer is 128 <- 32.
  - The bound families other than randn run on one row per form and direction, through the plane entry; the f32-operand
    entries add tiny on one g9, one 3x3 ks and one 1x1 ks row.  g1 carries them on its Kc = 64 row (BOUND_ROWS).
  - The f32-operand forward runs a fourth time through stk_conv2d_fwd_rec_f32 (the caller's records), bit-equal too.
  - Planes and their record are not Guarded (the kernels' 16-byte DMA reads need the allocation's alignment); they are
    compared with a copy after the launches instead.  Every other operand, output and scratch buffer is Guarded.
  - With the plain-C checker standing in, the exact families are held to the bound: the checker multiplies the decoded
    planes in full, lo lo included."""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import torch

import _conv_split_ref as cr
from _stream_util import Guarded
from _util import call, dev_of

Row = namedtuple('Row', 'name form taps N Kc M H W layout dirs C1 S1 entries')


def _row(name, form, taps, N, Kc, M, H, W, layout=0, dirs='fd', C1=0, S1=0, entries=('pl',)):
  return Row(name, form, taps, N, Kc, M, H, W, layout, dirs, C1, S1, entries)


BOTH = ('pl', 'f32')
ROWS = [
  # name, form, taps, N, Kc, M, H, W
  _row('h16', 'h16', 9, 96, 32, 128, 16, 16, dirs='f'),                  # 192 tiles, one chunk per tap
  _row('h16_dead', 'h16', 9, 96, 32, 96, 16, 16, dirs='f'),              # 32 dead rows in the tile
  _row('h16_two', 'h16', 9, 96, 32, 128, 16, 16, dirs='d', C1=32),       # dx1 32 rows + dx2 96 rows
  _row('h16_ragged', 'h16', 9, 96, 32, 136, 16, 16, dirs='d', C1=96),    # C1 96 + C2 40: the second row tile ragged
  _row('h32', 'h32', 9, 24, 64, 128, 32, 32),
  _row('h64', 'h64', 9, 6, 32, 128, 64, 64),
  _row('h64_two_tiles', 'h64', 9, 3, 32, 256, 64, 64, C1=160),           # two row tiles
  _row('g9_8x8', 'g9', 9, 384, 32, 128, 8, 8, entries=BOTH),             # W is no halo width; 2 images per tile
  _row('g9_12x20', 'g9', 9, 104, 32, 160, 12, 20, C1=96, entries=BOTH),  # ragged pixel tiles, 160 rows
  _row('g9_3x3', 'g9', 9, 2731, 32, 128, 3, 3, entries=BOTH),            # > 9 images per tile (unstaged temb), last tile ragged
  _row('g9_2x2', 'g9', 9, 6144, 32, 128, 2, 2, entries=BOTH),            # 32 images per tile
  _row('g9_src2', 'g9', 9, 384, 96, 128, 8, 8, dirs='f', S1=32, entries=('f32',)),      # sources 32 + 64
  _row('g1', 'g1', 1, 96, 32, 128, 16, 16, entries=BOTH),
  _row('g1_nin', 'g1', 1, 96, 32, 128, 16, 16, layout=1, entries=BOTH),
  _row('g1_12x20', 'g1', 1, 104, 64, 160, 12, 20, entries=BOTH),
  _row('ks_14+13', 'ks', 9, 2, 96, 96, 8, 8, C1=64, entries=BOTH),       # 1 tile, 27 chunks
  _row('ks_4x13+11', 'ks', 9, 1, 224, 128, 4, 4, entries=BOTH),          # 16 pixels in a 128-pixel tile, 63 chunks
  _row('ks_even', 'ks', 9, 8, 128, 128, 32, 32, entries=BOTH),           # 3 x 12
  _row('ks_src2', 'ks', 9, 2, 128, 96, 8, 8, dirs='f', S1=96, entries=('f32',)),        # sources 96 + 32: 3 x 12
  _row('ks1_7+6', 'ks', 1, 8, 416, 128, 16, 16, entries=BOTH),
  _row('ks1_6+6', 'ks', 1, 8, 384, 128, 16, 16, entries=BOTH),
  _row('ks1_nin', 'ks', 1, 8, 416, 128, 16, 16, layout=1, entries=BOTH),
]
BY_ROW = {r.name: r for r in ROWS}
EXPECTED_SPLITS = {'ks_14+13': (14, 13), 'ks_4x13+11': (13, 13, 13, 13, 11), 'ks_even': (12, 12, 12), 'ks_src2': (12, 12, 12),
                   'ks1_7+6': (7, 6), 'ks1_6+6': (6, 6), 'ks1_nin': (7, 6)}
# the smallest row of every (form, taps) that carries the bound families, per direction.  g1 takes its Kc = 64 row: with 32
# contracted terms the floor's worst case (every element half an fp16 step off, all of one sign) is within reach of the
# largest of 10^5 random draws, so no arithmetic, however right, keeps the model's HALF-bound margin in the faint family.
BOUND_ROWS = {'f': ('h16_dead', 'h32', 'h64', 'g9_8x8', 'g1_12x20', 'ks_14+13', 'ks1_7+6'),
              'd': ('h16_ragged', 'h32', 'h64', 'g9_8x8', 'g1_12x20', 'ks_14+13', 'ks1_7+6')}
EXACT_FAMILIES = ('exact', 'exact-ep')
BOUND_FAMILIES = ('randn', 'spread', 'faint', 'pow2', 'tiny', 'huge', 'wtiny')
FAMILIES = EXACT_FAMILIES + BOUND_FAMILIES
FORMS = ('h16', 'h32', 'h64', 'g9', 'g1', 'ks9', 'ks1')

Case = namedtuple('Case', 'row d entry fam')


def case_name(c):
  return f'{c.row}_{"dgrad" if c.d == "d" else "fwd"}_{c.entry}_{c.fam}'


def _cases():
  """ordered (row, direction, family, entry): the two entries of one set of operands are neighbours (one cached reference)"""
  out = []
  for r in ROWS:
    for d in r.dirs:
      fams = {e: list(EXACT_FAMILIES) + ['randn'] for e in r.entries}
      if r.name in BOUND_ROWS[d] and 'pl' in fams:
        fams['pl'] += [f for f in BOUND_FAMILIES if f != 'randn']
      if r.name in ('g9_8x8', 'ks_14+13', 'ks1_7+6') and 'f32' in fams:
        fams['f32'] += ['tiny']
      if r.name == 'g9_src2':
        fams['f32'] += ['src2x1e4']                    # the second source at 1e4 times the first
      for f in FAMILIES + ('src2x1e4',):
        out += [Case(r.name, d, e, f) for e in r.entries if f in fams[e]]
  return out


CASES = _cases()
IDS = [case_name(c) for c in CASES]
BY_NAME = dict(zip(IDS, CASES))


# ---- the plan restated (csrc/conv.hip split_plan, csrc/conv_x2d.h halo_ok) -------------------------------------------------
def cdiv(a, b):
  return -(-a // b)


def plan(r, entry='pl'):
  """(form, chunk counts of the K splits) of a row, or None where the split path refuses it."""
  Ng = r.N * r.H * r.W
  if not (r.Kc % 32 == 0 and r.M >= 96 and (r.S1 == 0 or r.S1 % 32 == 0)):
    return None
  tiles = cdiv(r.M, 128) * cdiv(Ng, 128)
  nch = r.taps * (r.Kc // 32)
  if tiles >= 192:
    halo = entry == 'pl' and r.taps == 9 and r.W in (16, 32, 64) and (r.H * r.W) % 128 == 0
    return (f'h{r.W}' if halo else ('g9' if r.taps == 9 else 'g1')), (nch,)
  splits = min(512 // tiles, nch // (12 if r.taps == 9 else 6))
  if (tiles < 16 and r.taps != 9) or splits < 2:
    return None
  cps = cdiv(nch, splits)
  n = cdiv(nch, cps)
  return 'ks', tuple(min(cps, nch - z * cps) for z in range(n))


def form_key(r):
  return ('ks9' if r.taps == 9 else 'ks1') if r.form == 'ks' else r.form


def layer(r, d):
  """(C1, C2, Cout) of the layer behind a row and direction: the C-ABI's view."""
  if d == 'f':
    return (r.S1, r.Kc - r.S1, r.M) if r.S1 else (r.Kc, 0, r.M)
  return (r.C1, r.M - r.C1, r.Kc) if r.C1 else (r.M, 0, r.Kc)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _randn(shape, seed):
  return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).numpy()


def _with_max(t, m):
  """t rescaled so that its largest magnitude is exactly m"""
  t = (t / np.abs(t).max()).astype(np.float32) * np.float32(m)
  assert np.abs(t).max() == np.float32(m)
  return t.astype(np.float32)


def _dyadic(shape, top, seed):
  """multiples of 1 / 4 in [-top, top]"""
  return (np.random.default_rng(seed).integers(-4 * top, 4 * top + 1, shape) / 4.0).astype(np.float32)


@functools.lru_cache(maxsize=4)
def inputs(name):
  """the operands of a case as numpy float32: a (activation operand), w (the weight tensor in its layout), and the
  epilogue's tensors (None where absent); temb is the WIDE tensor [N, M + 24], read at columns [8, 8 + M)."""
  c = BY_NAME[name]
  r = BY_ROW[c.row]
  K = 3 if r.taps == 9 else 1
  dgrad = c.d == 'd'
  C1, C2, Cout = layer(r, c.d)
  Cin = C1 + C2
  wshape = (Cin, Cout) if r.layout == 1 else (Cout, Cin, K, K)
  ashape, oshape = (r.N, r.Kc, r.H, r.W), (r.N, r.M, r.H, r.W)
  t = dict(bias=None, temb=None, res=None, div=1.0, alpha=1.0, beta=(0.0, 0.0), dx0=None)
  if c.fam in EXACT_FAMILIES:
    hmax = 2 if r.Kc * r.taps <= 864 else 1
    t['a'], t['w'] = cr.exact_tensor(ashape, hmax, 1), cr.exact_tensor(wshape, hmax, 2)
    if c.fam == 'exact-ep':
      if dgrad:
        t.update(alpha=0.5, beta=(0.5, 0.0), dx0=_dyadic(oshape, 4, 5))
      else:
        t.update(bias=_dyadic((r.M,), 2, 3), temb=_dyadic((r.N, r.M + 24), 2, 4), res=_dyadic(oshape, 4, 5), div=2.0)
  else:
    a = _randn(ashape, 11)
    w = _randn(wshape, 13) / np.float32(np.sqrt(r.Kc * r.taps))
    if c.fam == 'randn':
      if dgrad:
        t.update(alpha=0.5, beta=(0.0, 0.75) if r.C1 else (0.25, 0.0), dx0=_randn(oshape, 15))
      else:
        t.update(bias=_randn((r.M,), 14), temb=_randn((r.N, r.M + 24), 15), res=_randn(oshape, 16),
                 div=float(np.float32(np.sqrt(2.0))))
    elif c.fam == 'spread':
      f = np.logspace(-4, 0, r.N)[np.random.default_rng(3).permutation(r.N)]
      a = a * f.astype(np.float32)[:, None, None, None]
    elif c.fam == 'faint':
      a[r.N - 1] *= np.float32(2.0 ** -30)
    elif c.fam == 'pow2':
      a = np.clip(a, -3.9, 3.9)
      a[r.N - 1, r.Kc // 2, r.H // 2, r.W - 1] = -4.0
    elif c.fam == 'tiny':
      a, w = _with_max(a, 2.0 ** -60), _with_max(w, 2.0 ** -50)
    elif c.fam == 'huge':
      a, w = _with_max(a, 2.0 ** 40), _with_max(w, 2.0 ** 20)
    elif c.fam == 'wtiny':
      w = _with_max(w, 2.0 ** -100)
    elif c.fam == 'src2x1e4':
      a[:, r.S1:] *= np.float32(1e4)
    else:
      raise KeyError(c.fam)
    t['a'], t['w'] = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(w, np.float32)
  if dgrad and t['dx0'] is not None and r.C1 and t['beta'][1] == 0.0:
    t['dx0'][:, r.C1:] = np.nan                      # never read
  if dgrad and t['dx0'] is not None and t['beta'][0] == 0.0:
    t['dx0'][:, :(r.C1 or r.M)] = np.nan
  return t


def problem_of(name):
  c = BY_NAME[name]
  r = BY_ROW[c.row]
  t = inputs(name)
  C1, C2, Cout = layer(r, c.d)
  K = 3 if r.taps == 9 else 1
  W = cr.gemm_weights(t['w'], r.layout, C1 + C2, Cout, K, c.d == 'd')
  temb = None if t['temb'] is None else np.ascontiguousarray(t['temb'][:, 8:8 + r.M])
  return cr.problem(c.d == 'd', t['a'], W, r.taps, plan(r, c.entry)[1], t['bias'], temb, t['res'], t['div'], t['alpha'],
                    r.C1 or r.M, t['beta'], t['dx0'], r.S1 or r.Kc)


@functools.lru_cache(maxsize=2)
def _exact_acc(row, d):
  name = next(n for n, c in BY_NAME.items() if (c.row, c.d, c.fam) == (row, d, 'exact'))
  return cr.three_term_acc(problem_of(name))


@functools.lru_cache(maxsize=2)
def _parts(row, d, fam):
  name = next(n for n, c in BY_NAME.items() if (c.row, c.d, c.fam) == (row, d, fam))
  return cr.parts(problem_of(name))


def three_term_of(name):
  """three_term() of a whole exact case; 'exact' and 'exact-ep', planes and f32 entry share operands and so the contraction"""
  c = BY_NAME[name]
  return cr.three_term(problem_of(name), acc=_exact_acc(c.row, c.d))


def reference_of(name):
  """(reference, bound) of a whole case, from one cached set of float64 contractions per (row, direction, family)"""
  c = BY_NAME[name]
  fam = 'exact' if c.fam in EXACT_FAMILIES else c.fam
  p, pt = problem_of(name), _parts(c.row, c.d, fam)
  return cr.reference(p, pt=pt), cr.bound(p, pt=pt)


def model_subset(name):
  """images and pixels the numpy model covers: both ends of the batch with their neighbours (tiles that straddle images,
  the faint last image), all pixels of a small map"""
  r = BY_ROW[BY_NAME[name].row]
  idx = sorted({0, 1, r.N - 2, r.N - 1} & set(range(r.N))) if r.H * r.W <= 256 else sorted({0, r.N - 1})
  return idx, cr.pixels_of(r.H, r.W)


# ---- the runners -----------------------------------------------------------------------------------------------------------
class _WprepDesc(ctypes.Structure):       # StkWprepDesc of include/stk.h
  _fields_ = [('w', ctypes.c_void_p), ('wp', ctypes.c_void_p), ('sm', ctypes.c_long), ('sk', ctypes.c_long),
              ('M', ctypes.c_int), ('Kc', ctypes.c_int), ('Mpad', ctypes.c_int), ('taps', ctypes.c_int),
              ('flip', ctypes.c_int), ('reserved', ctypes.c_int)]


def assert_form(lib, c):
  """the library's own diagnostics name the form the row was written for (device only: the checker has one form)"""
  r = BY_ROW[c.row]
  K = 3 if r.taps == 9 else 1
  C1, C2, Cout = layer(r, c.d)
  di = 1 if c.d == 'd' else 0
  form, splits = plan(r, c.entry)
  assert form == r.form and (form != 'ks' or splits == EXPECTED_SPLITS[r.name]), (r.name, form, splits)
  if c.entry == 'pl':
    assert int(lib.conv2d_pl_ok(di, C1, C2, r.N, r.H, r.W, Cout, K, K, 1, K // 2)) == 1, c
  if not lib.is_device:
    return
  assert int(lib.conv2d_variant(di, C1, C2, r.N, r.H, r.W, Cout, r.H, r.W, K, K, 1, K // 2, r.layout)) == 5, c
  if c.entry == 'pl':
    ks = int(lib.conv2d_pl_ksplit(di, C1, C2, r.N, r.H, r.W, Cout, K, K))
    halo = int(lib.conv2d_pl_halo(di, C1, C2, r.N, r.H, r.W, Cout, K, K))
    got = (f'h{halo}' if halo else ('g9' if K == 3 else 'g1')) if ks == 1 else 'ks'
    assert (got, ks) == (form, len(splits)), (c, got, ks, form, splits)
  else:          # the f32-operand entry runs the same plan; its scratch holds the K-split slabs
    fn = lib.conv2d_dgrad_ws_bytes if di else lib.conv2d_fwd_ws_bytes
    nb = int(fn(C1, C2, r.N, r.H, r.W, Cout, K, K, 1, K // 2))
    slabs = len(splits) * r.M * r.N * r.H * r.W * 4 if len(splits) > 1 else 0
    fixed = 255 + 256 * 3 + 256 * 2 * 4 + 2 * 2 * r.taps * cdiv(r.M, 128) * 128 * r.Kc     # split_ws: header, planes, records, roundings
    assert slabs < nb <= slabs + fixed, (c, nb, slabs, fixed)


def _nan_like(shape):
  return np.full(shape, np.nan, np.float32)


def _bytes(n):
  return torch.full((max(int(n), 16),), 0xFF, dtype=torch.uint8)          # 0xFFFFFFFF: a NaN in every float of the scratch


def run(lib, name):
  """Three launches of one case on Guarded buffers -- twice with wp = NULL, once on weights prepared by
  stk_conv2d_wprep_batch (device only) -- which must agree bit for bit; NaN-prefilled outputs and scratch of exactly the
  reported size; no sentinel written, no operand changed.  Returns the result as numpy [N, M, H, W] (the data gradient's
  two destinations joined along the rows)."""
  c = BY_NAME[name]
  r = BY_ROW[c.row]
  t = inputs(name)
  d = dev_of(lib)
  K = 3 if r.taps == 9 else 1
  dgrad = c.d == 'd'
  di = 1 if dgrad else 0
  C1, C2, Cout = layer(r, c.d)
  Cin = C1 + C2
  dims = (C1, C2, r.N, r.H, r.W, Cout, K, K, 1, K // 2)
  nb = int((lib.conv2d_dgrad_ws_bytes if dgrad else lib.conv2d_fwd_ws_bytes)(*dims))
  assert nb > 0 or not lib.is_device
  a, w = t['a'], t['w']
  if c.entry == 'f32' and not dgrad and C2:
    srcs = [np.ascontiguousarray(a[:, :C1]), np.ascontiguousarray(a[:, C1:])]
  else:
    srcs = [a]
  g_src = [Guarded(s, d) for s in srcs]
  g_w = Guarded(w, d)
  g_in = {k: Guarded(t[k], d) for k in ('bias', 'temb', 'res') if t[k] is not None}
  operands = list(zip(g_src, srcs)) + [(g_w, w)] + [(g_in[k], t[k]) for k in g_in]
  planes = rec = None
  if c.entry == 'pl':
    rec = torch.zeros(256, device=d)
    call(lib, 'amax_partial_f32', g_src[0].view, a.size, rec)
    planes = torch.zeros(int(lib.planes_bytes(r.N, r.Kc, r.H * r.W)), dtype=torch.uint8, device=d)
    call(lib, 'split_planes_f32', g_src[0].view, r.N, r.Kc, r.H * r.W, rec, 256, planes)
    planes0, rec0 = planes.clone(), rec.clone()

  def prepared():
    nbw = int(lib.conv2d_wp_bytes(di, *dims))
    assert nbw > 0, ('no prepared-weight block', c)
    blk = torch.full((nbw + 256,), 0xff, dtype=torch.uint8, device=d)
    ptr = (blk.data_ptr() + 255) // 256 * 256
    desc = _WprepDesc()
    n = lib.conv2d_wp_desc(di, g_w.view.data_ptr(), r.layout, Cin, Cout, K, K, ptr, ctypes.byref(desc))
    assert n > 0
    table = torch.from_numpy(np.frombuffer(bytes(desc), dtype=np.uint8).copy()).to(d)
    call(lib, 'conv2d_wprep_batch', table, 1, n)
    return blk, ptr

  def launch(wp):
    ws = Guarded(_bytes(nb), d)
    if dgrad:
      outs = []
      for rows, b in ((slice(0, C1), t['beta'][0]), (slice(C1, Cin), t['beta'][1])):
        if rows.stop > rows.start:
          outs.append(Guarded(np.ascontiguousarray(t['dx0'][:, rows]) if b != 0.0 else _nan_like((r.N, rows.stop - rows.start, r.H, r.W)), d))
      dx2 = outs[1].view if C2 else None
      tail = (outs[0].view, C1, t['beta'][0], dx2, C2, t['beta'][1], t['alpha'], r.N, r.H, r.W, Cout)
      if c.entry == 'pl':
        call(lib, 'conv2d_dgrad_pl_f32', planes, rec, g_w.view, r.layout, *tail, K, K, wp, ws.view, nb)
      elif wp is None:
        call(lib, 'conv2d_dgrad_f32', g_src[0].view, g_w.view, r.layout, *tail, r.H, r.W, K, K, 1, K // 2, ws.view, nb)
      else:
        call(lib, 'conv2d_dgrad_wp_f32', g_src[0].view, g_w.view, r.layout, *tail, r.H, r.W, K, K, 1, K // 2, wp, None, ws.view, nb)
    else:
      outs = [Guarded(_nan_like((r.N, r.M, r.H, r.W)), d)]
      tptr, tstride = (g_in['temb'].view.data_ptr() + 4 * 8, r.M + 24) if 'temb' in g_in else (None, 0)
      ep = (g_w.view, r.layout, g_in['bias'].view if 'bias' in g_in else None, tptr, tstride,
            g_in['res'].view if 'res' in g_in else None, t['div'], outs[0].view, r.N, r.H, r.W, Cout)
      if c.entry == 'pl':
        call(lib, 'conv2d_fwd_pl_f32', planes, rec, r.Kc, *ep, K, K, wp, ws.view, nb)
      else:
        x2 = g_src[1].view if C2 else None
        if wp is None:
          call(lib, 'conv2d_fwd_f32', g_src[0].view, C1, x2, C2, *ep, r.H, r.W, K, K, 1, K // 2, ws.view, nb)
        elif wp == 'rec':        # the caller's records already hold the maxima of both sources (stk_conv2d_fwd_rec_f32)
          amax = torch.full((768,), float('nan'), device=d)
          call(lib, 'amax_partial_f32', g_src[0].view, srcs[0].size, amax[:256])
          if C2:
            call(lib, 'amax_partial_f32', g_src[1].view, srcs[1].size, amax[256:512])
          call(lib, 'conv2d_fwd_rec_f32', g_src[0].view, C1, x2, C2, *ep, r.H, r.W, K, K, 1, K // 2, None, amax, ws.view, nb)
        else:
          call(lib, 'conv2d_fwd_wp_f32', g_src[0].view, C1, x2, C2, *ep, r.H, r.W, K, K, 1, K // 2, wp, None, ws.view, nb)
    if lib.is_device:
      torch.cuda.synchronize()
    for g in outs + [ws]:
      g.check(name)
    return np.concatenate([g.view.cpu().numpy() for g in outs], 1)

  runs = [launch(None), launch(None)]
  if lib.is_device:
    blk, ptr = prepared()
    runs.append(launch(ptr))
    del blk
  if c.entry == 'f32' and not dgrad:
    runs.append(launch('rec'))
  for i, o in enumerate(runs[1:], 1):
    assert np.array_equal(runs[0].view(np.int32), o.view(np.int32)), f'{name}: launch {i} differs from launch 0 ' \
        f'(0, 1: wp = NULL; then prepared weights on the device; then the record entry of the f32 forward)'
  for g, host in operands:
    g.check(name + ' operand')
    assert np.array_equal(g.view.cpu().numpy().view(np.int32), host.view(np.int32)), f'{name}: an operand was written'
  if planes is not None:
    assert torch.equal(planes, planes0) and torch.equal(rec, rec0), f'{name}: the planes or their record were written'
  return runs[0]
