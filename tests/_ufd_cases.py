"""upfirdn2d on every kernel route and parameter axis: cases, a float64 reference, the rounding bound, guarded buffers and a
model of the dispatch (tests/test_gpu_upfirdn2d.py on the HIP library, tests/test_upfirdn2d_cases_cpu.py on the plain-C
checker and on the definition itself).

Reference.  The definition of the operator (op/upfirdn2d.py:159-200 of the reference), in float64 torch on the CPU:
zero-insert (u[:, ::up_y, ::up_x] = x), F.pad by (pad_x0, pad_x1, pad_y0, pad_y1) -- negative values crop --, F.conv2d with
the flipped taps and stride (down_y, down_x), plus beta * old.  `minor` is folded into the planes by a permute.  The same
routine on |x|, |k|, |beta old| gives B, the sum of the absolute terms of every output element.

Bound (derived, not measured).  An output is beta * old plus at most kh kw products summed in fp32, in any order, with or
without FMA: every partial sum is bounded by B, so
  fp32   |err| <= (kh kw + 2) 2^-24 B          (kh kw products and additions of which at most kh kw + 1 round, beta old, sum)
  _f64   the same with 2^-53
  _f16   2^-11 |want| + (kh kw + 2) 2^-24 B + 2^-25      (fp32 accumulation, one rounding to half; 2^-25: half a subnormal)
element by element.  Where every tap of an output falls in the padding B = |beta old| and the bound is that tight.  The
half reference is computed from the fp16-rounded inputs and taps.  The double entry gets the fp32 values widened: their
products are exact in double, so the float64 reference has next to no error of its own and the 2^-53 bound is sound (a
kernel that accumulated in fp32 would miss it by 2^29); that double survives the entry at all is tests/_op_cases.py's check.

Inputs.  randn, plane p scaled by 10^e(p) with e spread over [-2, 2] and neighbouring planes far apart, so that a value
taken from a neighbouring plane's window is far outside the bound; taps are randn, NOT the symmetric binomial: a symmetric
FIR hides a flipped or transposed tap index.  Condition on the inputs (asserted in the CPU half): the definition evaluated
in float32 torch on the CPU stays within the fp32 bound on every case.

Buffers.  Input and taps lie in a larger buffer whose 64 leading and 64 trailing floats (256 bytes) are NaN, the payload on
a 16-byte boundary or one float past it: a read outside the tensor that reaches a result shows as NaN.  The output lies
between two guards of 256 bytes of a sentinel bit pattern that must be bit-identical after the launch; its payload starts
as NaN for beta == 0 (written, never read) and as random values otherwise.  Every overrun such a layout can catch stays
inside the test's own allocation.
"""
import collections

import torch
import torch.nn.functional as F

from _stream_util import U, place, within

GUARD_BYTES = 256                # 64 floats
SENTINEL = 0xA5                  # 0xA5A5A5A5 is a normal float, -2.87e-16: never NaN, never a plausible result
BETAS = (0.0, 0.5)
MAX_TAPS = 8
LDS_FLOATS = 12288

# ---- cases ----------------------------------------------------------------------------------------------------------
# params = (major, H, W, minor, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)
Case = collections.namedtuple('Case', 'name params one_in route types')


def _c(name, major, H, W, minor, taps, up, down, pad, route, one_in=False, types=False):
  up = up if isinstance(up, tuple) else (up, up)
  down = down if isinstance(down, tuple) else (down, down)
  return Case(name, (major, H, W, minor, taps[0], taps[1], up[0], up[1], down[0], down[1]) + tuple(pad), one_in, route, types)


T11, T12, T12D, T21 = 'tiled<1,1>', 'tiled<1,2>', 'tiled<1,2,deint>', 'tiled<2,1>'
CASES = [
  # taps other than 4 x 4, plain FIR: the generic inner loop of tiled<1,1> (every GaussianBlur of size 2 .. 8, box taps)
  _c('fir5', 3, 16, 16, 1, (5, 5), 1, 1, (2, 2, 2, 2), (T11, 'planes4/vec', 'loop'), types=True),
  _c('fir7', 3, 16, 16, 1, (7, 7), 1, 1, (3, 3, 3, 3), (T11, 'planes4/vec', 'loop')),
  _c('fir8_12x20', 2, 12, 20, 1, (8, 8), 1, 1, (4, 3, 3, 4), (T11, 'planes2/vec', 'loop')),
  _c('fir1', 2, 16, 16, 1, (1, 1), 1, 1, (0, 0, 0, 0), (T11, 'planes4/vec', 'loop')),
  _c('fir2', 2, 16, 16, 1, (2, 2), 1, 1, (1, 0, 0, 1), (T11, 'planes4/vec', 'loop')),
  _c('fir3x5', 2, 12, 16, 1, (3, 5), 1, 1, (2, 2, 1, 1), (T11, 'planes4/vec', 'loop'), types=True),
  _c('fir4x1', 2, 12, 16, 1, (4, 1), 1, 1, (0, 0, 2, 1), (T11, 'planes4/vec', 'loop')),
  _c('fir1x4', 2, 12, 16, 1, (1, 4), 1, 1, (2, 1, 0, 0), (T11, 'planes4/vec', 'loop')),
  _c('fir3_32', 2, 32, 32, 1, (3, 3), 1, 1, (1, 1, 1, 1), (T11, 'planes1/vec', 'loop')),
  _c('fir5_70_bands', 2, 70, 70, 1, (5, 5), 1, 1, (2, 2, 2, 2), (T11, 'bands/scalar', 'loop')),
  _c('fir5_260_tiles', 1, 10, 260, 1, (5, 5), 1, 1, (2, 2, 2, 2), (T11, 'tiles', 'loop')),
  _c('fir9_direct', 2, 16, 16, 1, (9, 9), 1, 1, (4, 4, 4, 4), ('direct', None, None)),
  # tiled<1,1>, 4 x 4 taps in registers
  _c('fir4_16', 2, 16, 16, 1, (4, 4), 1, 1, (2, 1, 2, 1), (T11, 'planes4/vec', 'k4')),
  _c('fir4_259_tiles', 1, 10, 259, 1, (4, 4), 1, 1, (2, 2, 2, 2), (T11, 'tiles', 'k4')),                 # 260 outputs per row
  _c('fir4_15x17_padxy', 2, 15, 17, 1, (4, 4), 1, 1, (3, 3, 0, 0), (T11, 'planes2/scalar', 'k4')),
  _c('fir5_one_in', 3, 16, 16, 1, (5, 5), 1, 1, (2, 2, 2, 2), (T11, 'planes4/scalar', 'loop'), one_in=True),
  # the flat-order kernel with other paddings than (2, 2) and (-1, -1)
  _c('flat_padxy', 2, 15, 18, 1, (4, 4), 1, 1, (2, 1, 1, 2), ('flat', 'planes4/scalar', None), types=True),
  _c('flat_257_wide', 1, 12, 258, 1, (4, 4), 1, 1, (1, 1, 2, 2), ('flat', 'planes1/scalar', None)),      # a 257-wide plane
  _c('flat_257_tall', 1, 44, 258, 1, (4, 4), 1, 1, (1, 1, 2, 2), ('flat', 'bands/scalar', None)),         # 45 x 257: bands of 4 rows
  _c('flat_13planes', 13, 8, 8, 1, (4, 4), 1, 1, (2, 2, 2, 2), ('flat', 'planes25/vec', None)),          # 25 per workgroup
  _c('flat_one_in', 2, 16, 16, 1, (4, 4), 1, 1, (2, 2, 2, 2), ('flat', 'planes4/scalar', None), one_in=True),
  # up-sampling by 2, four outputs per thread: every parity of pad_x0 and pad_y0
  _c('up_pad2112', 2, 16, 16, 1, (4, 4), 2, 1, (2, 1, 1, 2), (T21, 'planes4/vec', 'k4'), types=True),
  _c('up_pad3003', 2, 16, 16, 1, (4, 4), 2, 1, (3, 0, 0, 3), (T21, 'planes4/vec', 'k4')),
  _c('up_pad1230', 2, 16, 16, 1, (4, 4), 2, 1, (1, 2, 3, 0), (T21, 'planes4/vec', 'k4')),
  _c('up_crop', 2, 16, 16, 1, (4, 4), 2, 1, (-1, 2, 2, -1), (T21, 'planes4/vec', 'k4')),
  _c('up_one_in', 2, 16, 16, 1, (4, 4), 2, 1, (2, 1, 2, 1), (T21, 'planes4/scalar', 'k4'), one_in=True),
  _c('up_130_tiles', 1, 10, 130, 1, (4, 4), 2, 1, (2, 1, 1, 2), (T21, 'tiles', 'k4')),                   # 260 outputs per row
  _c('up_131_tiles', 1, 10, 131, 1, (4, 4), 2, 1, (1, 2, 2, 1), (T21, 'tiles', 'k4')),                   # 262
  _c('up6_bands', 2, 40, 40, 1, (6, 6), 2, 1, (3, 2, 3, 2), (T21, 'bands/vec', 'loop')),
  _c('up2_tiles', 1, 20, 140, 1, (2, 2), 2, 1, (1, 0, 1, 0), (T21, 'tiles', 'loop')),
  _c('up_1plane', 1, 8, 8, 1, (4, 4), 2, 1, (2, 1, 2, 1), (T21, 'planes2/vec', 'loop')),                 # major = 1
  # down-sampling by 2, rows kept interleaved
  _c('down_32', 2, 32, 32, 1, (4, 4), 1, 2, (1, 1, 1, 1), (T12, 'planes4/vec', 'k4')),
  _c('down_pad1120', 2, 16, 16, 1, (4, 4), 1, 2, (1, 1, 2, 0), (T12, 'planes4/vec', 'loop')),
  _c('down_pad0211', 2, 16, 16, 1, (4, 4), 1, 2, (0, 2, 1, 1), (T12, 'planes4/vec', 'loop'), types=True),
  _c('down_crop', 2, 16, 16, 1, (4, 4), 1, 2, (-1, 0, 1, -2), (T12, 'planes4/vec', 'loop')),
  _c('down_17x15', 3, 17, 15, 1, (4, 4), 1, 2, (1, 1, 1, 1), (T12, 'planes4/scalar', 'loop')),
  _c('down_one_in', 2, 32, 32, 1, (4, 4), 1, 2, (1, 1, 1, 1), (T12, 'planes4/scalar', 'k4'), one_in=True),
  _c('down_520_tiles', 1, 20, 520, 1, (4, 4), 1, 2, (1, 1, 1, 1), (T12, 'tiles', 'k4')),                 # 260 outputs per row
  _c('down_522_tiles', 1, 20, 522, 1, (4, 4), 1, 2, (0, 2, 2, 0), (T12, 'tiles', 'k4')),                 # 261
  _c('down_520_short', 1, 12, 520, 1, (4, 4), 1, 2, (1, 1, 1, 1), (T12, 'tiles', 'loop')),               # 6 rows: two outputs per thread
  # down-sampling by 2, rows de-interleaved (128 and 256 outputs per row)
  _c('deint_256', 2, 12, 256, 1, (4, 4), 1, 2, (1, 1, 1, 1), (T12D, 'planes1/vec', 'k4')),
  _c('deint_255', 1, 12, 255, 1, (4, 4), 1, 2, (1, 2, 1, 1), (T12D, 'planes1/scalar', 'k4')),
  _c('deint_bands', 1, 40, 160, 1, (4, 4), 1, 2, (2, 0, 0, 2), (T12D, 'bands/vec', 'k4')),
  _c('deint_fir3', 1, 9, 300, 1, (3, 3), 1, 2, (1, 1, 1, 1), (T12D, 'planes1/vec', 'loop')),
  _c('deint_fir6', 1, 24, 256, 1, (6, 6), 1, 2, (2, 2, 2, 2), (T12D, 'planes1/vec', 'loop')),
  # the direct kernel: unequal factors, minor > 1, other factors, planes too small for a tile
  _c('ux2_uy1', 2, 12, 10, 1, (4, 4), (2, 1), 1, (2, 1, 1, 2), ('direct', None, None), types=True),
  _c('ux1_uy2', 2, 12, 10, 1, (4, 4), (1, 2), 1, (1, 2, 2, 1), ('direct', None, None), types=True),
  _c('dx2_dy1', 2, 12, 10, 1, (4, 4), 1, (2, 1), (1, 1, 2, 1), ('direct', None, None), types=True),
  _c('dx1_dy2', 2, 12, 10, 1, (4, 4), 1, (1, 2), (2, 1, 1, 1), ('direct', None, None), types=True),
  _c('minor3_up', 2, 12, 10, 3, (4, 4), 2, 1, (2, 1, 2, 1), ('direct', None, None), types=True),
  _c('minor5_down', 2, 12, 10, 5, (4, 4), 1, 2, (1, 1, 1, 1), ('direct', None, None), types=True),
  _c('up2_down2', 2, 12, 10, 1, (4, 4), 2, 2, (2, 1, 1, 2), ('direct', None, None)),
  _c('down3', 2, 12, 10, 1, (5, 3), 1, 3, (1, 2, 2, 2), ('direct', None, None)),
  _c('up4', 2, 12, 10, 1, (8, 8), 4, 1, (5, 2, 4, 3), ('direct', None, None)),
  _c('small_16', 1, 16, 16, 1, (4, 4), 1, 2, (1, 1, 1, 1), ('direct', None, None)),
  _c('small_7x8', 7, 8, 8, 1, (4, 4), 1, 2, (1, 1, 1, 1), ('direct', None, None)),
]
IDS = [c.name for c in CASES]
TYPE_IDS = [c.name for c in CASES if c.types]

# every (kernel, staging, inner) the cases must reach: csrc/upfirdn2d.hip's kernels in each staging form and inner loop
ROUTES = {
  ('direct', None, None),
  ('flat', 'planes4/scalar', None), ('flat', 'planes25/vec', None), ('flat', 'planes1/scalar', None), ('flat', 'bands/scalar', None),
  (T11, 'planes4/vec', 'loop'), (T11, 'planes2/vec', 'loop'), (T11, 'planes1/vec', 'loop'), (T11, 'bands/scalar', 'loop'),
  (T11, 'tiles', 'loop'), (T11, 'planes4/scalar', 'loop'), (T11, 'planes4/vec', 'k4'), (T11, 'planes2/scalar', 'k4'), (T11, 'tiles', 'k4'),
  (T21, 'planes4/vec', 'k4'), (T21, 'planes4/scalar', 'k4'), (T21, 'tiles', 'k4'),
  (T21, 'bands/vec', 'loop'), (T21, 'tiles', 'loop'), (T21, 'planes2/vec', 'loop'),
  (T12, 'planes4/vec', 'k4'), (T12, 'planes4/vec', 'loop'), (T12, 'planes4/scalar', 'loop'), (T12, 'planes4/scalar', 'k4'),
  (T12, 'tiles', 'k4'), (T12, 'tiles', 'loop'),
  (T12D, 'planes1/vec', 'k4'), (T12D, 'planes1/scalar', 'k4'), (T12D, 'bands/vec', 'k4'), (T12D, 'planes1/vec', 'loop'),
}


def _axes():
  """name -> predicate on a Case: every value of a parameter axis the case list must keep."""
  A = {}
  P = lambda c: dict(zip('major H W minor kh kw ux uy dx dy px0 px1 py0 py1'.split(), c.params))
  A['pad_x0 != pad_y0'] = lambda c: P(c)['px0'] != P(c)['py0']
  A['pad_x1 != pad_y1'] = lambda c: P(c)['px1'] != P(c)['py1']
  A['negative pad0'] = lambda c: P(c)['px0'] < 0
  A['negative pad1'] = lambda c: P(c)['py1'] < 0
  for t in ((1, 1), (2, 2), (3, 3), (3, 5), (4, 1), (1, 4), (4, 4), (5, 5), (5, 3), (6, 6), (7, 7), (8, 8), (9, 9)):
    A[f'taps {t[0]}x{t[1]}'] = lambda c, t=t: c.params[4:6] == t
  A['up_x > up_y'] = lambda c: P(c)['ux'] > P(c)['uy']
  A['up_x < up_y'] = lambda c: P(c)['ux'] < P(c)['uy']
  A['down_x > down_y'] = lambda c: P(c)['dx'] > P(c)['dy']
  A['down_x < down_y'] = lambda c: P(c)['dx'] < P(c)['dy']
  A['up 2 and down 2'] = lambda c: c.params[6:10] == (2, 2, 2, 2)
  A['down 3'] = lambda c: c.params[8:10] == (3, 3)
  A['up 4'] = lambda c: c.params[6:8] == (4, 4)
  A['minor 3 with up 2'] = lambda c: P(c)['minor'] == 3 and P(c)['ux'] == 2
  A['minor 5 with down 2'] = lambda c: P(c)['minor'] == 5 and P(c)['dx'] == 2
  for k in (T11, T12, T21, 'flat'):
    A[f'{k} entered one float in'] = lambda c, k=k: c.one_in and c.route[0] == k
  # the four-outputs-per-thread up-sampling decides its tap phase from the parity of ox - pad_x0 and oy - pad_y0
  for px in (0, 1):
    for py in (0, 1):
      A[f'up 2 k4, pad_x0 % 2 = {px}, pad_y0 % 2 = {py}'] = lambda c, px=px, py=py: (
        c.route[0] == T21 and c.route[2] == 'k4' and P(c)['px0'] % 2 == px and P(c)['py0'] % 2 == py)
  A['more than 256 outputs per row, not a multiple of 4'] = lambda c: c.route[1] == 'tiles' and out_hw(c.params)[1] % 4 != 0
  A['more planes per workgroup than planes'] = lambda c: c.route[1] is not None and c.route[1].startswith('planes') and (
    int(c.route[1].split('/')[0][6:]) > P(c)['major'])
  A['one plane'] = lambda c: P(c)['major'] == 1
  A['types: unequal factors'] = lambda c: c.types and (P(c)['ux'] != P(c)['uy'] or P(c)['dx'] != P(c)['dy'])
  A['types: minor > 1'] = lambda c: c.types and P(c)['minor'] > 1
  A['types: kh != kw'] = lambda c: c.types and P(c)['kh'] != P(c)['kw']
  A['types: pad_x != pad_y'] = lambda c: c.types and P(c)['px0'] != P(c)['py0']
  return A


AXES = _axes()


def out_hw(params):
  """The output extent, by floor division (the reference's Python and op.upfirdn2d.FirMap.of); None where either
  numerator is negative: the entries return STK_EINVAL there."""
  major, H, W, minor, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1 = params
  nh, nw = H * uy + py0 + py1 - kh, W * ux + px0 + px1 - kw
  if nh < 0 or nw < 0:
    return None
  return nh // dy + 1, nw // dx + 1


# ---- route model ----------------------------------------------------------------------------------------------------
def _deint(down, tow_log2):
  return down == 2 and tow_log2 >= 7


def _pitch(cols, deint):
  return 2 * ((((cols + 1) >> 1) + 3) & ~3) if deint else cols | 1


def route(params, aligned=True):
  """(kernel, staging, inner) that launch() of csrc/upfirdn2d.hip takes for the fp32 entries: a restatement of its shape
  rules.  The library has no predicate or query to cross-check this against, so it is only as good as the reading it
  was written from: it pins which cases were CHOSEN for which route, and the per-element comparison stands whatever route
  a case really takes.
    kernel   'direct', 'flat', 'tiled<1,1>', 'tiled<1,2>', 'tiled<1,2,deint>', 'tiled<2,1>'
    staging  'planesN/vec|scalar' (N whole planes per workgroup, one contiguous run), 'bands/vec|scalar' (a band of rows of
             one plane, a run too), 'tiles' (a 64-wide tile, element by element); None for direct
    inner    'k4' (4 x 4 taps in registers, four outputs per thread) or 'loop'; None for direct and flat"""
  major, H, W, minor, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1 = params
  oh, ow = out_hw(params)
  cdiv = lambda a, b: -(-a // b)
  tiled_ok = (minor == 1 and ux == uy and dx == dy and kh <= MAX_TAPS and kw <= MAX_TAPS and
              ((ux == 1 and dx in (1, 2)) or (ux == 2 and dx == 1)))
  run_vec = (H * W) % 4 == 0 and W % 4 == 0 and aligned
  form = lambda v: 'vec' if v else 'scalar'
  if tiled_ok and ux == 1 and dx == 1 and kh == 4 and kw == 4 and ow % 4 != 0 and ow + 3 <= 1024 and oh * ow < 1 << 21:
    pitch = (ow + 3) | 1
    toh, ppb = oh, 1
    plane_win = (((oh + 3) & ~3) + 3) * pitch
    if plane_win <= LDS_FLOATS:
      ppb = max(2048 // (oh * ow), 1)
      while ppb > 1 and (ppb * plane_win > LDS_FLOATS or ppb > 2 * major):
        ppb -= 1
    else:
      toh = max(max(2048 // ow, 1) & ~3, 4)
      while toh > 4 and (toh + 3) * pitch > LDS_FLOATS:
        toh -= 4
    tiles_y = cdiv(oh, toh)
    win = (((toh + 3) & ~3) + 3) * pitch
    if win * ppb <= LDS_FLOATS:
      return 'flat', (f'planes{ppb}' if tiles_y == 1 else 'bands') + '/' + form(run_vec), None
  if tiled_ok:
    up, down = ux, dx
    tow_max = 8 if ow <= 256 else 6
    tow_log2 = toh_log2 = 2
    while tow_log2 < tow_max and (1 << tow_log2) < ow:
      tow_log2 += 1
    wide = (1 << tow_log2) >= ow
    out_log2 = 10
    if wide and up == 2:
      out_log2 = 12
    elif wide and down == 2 and oh > (1 << (10 - tow_log2)):
      out_log2 = 11
    while toh_log2 + tow_log2 < out_log2 and (1 << toh_log2) < oh:
      toh_log2 += 1
    deint = _deint(down, tow_log2)

    def win_floats(th_log2):
      r = (((1 << th_log2) - 1) * down + kh - 1) // up + 2
      c = (((1 << tow_log2) - 1) * down + kw - 1) // up + 2
      return r * _pitch(c, deint)
    while toh_log2 > 2 and win_floats(toh_log2) > LDS_FLOATS:
      toh_log2 -= 1
    tiles_x, tiles_y = cdiv(ow, 1 << tow_log2), cdiv(oh, 1 << toh_log2)
    whole = tiles_x == 1
    ppb_log2 = max(out_log2 - tow_log2 - toh_log2, 0) if tiles_x * tiles_y == 1 else 0
    win = win_floats(toh_log2)
    while ppb_log2 > 0 and ((win << ppb_log2) > LDS_FLOATS or (1 << ppb_log2) > 2 * major):
      ppb_log2 -= 1
    nq = (1 << (ppb_log2 + tow_log2 + toh_log2)) >> 8
    if win <= LDS_FLOATS and nq >= 1:
      k4 = kh == 4 and kw == 4 and nq % 4 == 0
      kernel = T11 if down == 1 and up == 1 else T21 if up == 2 else T12D if deint else T12
      if not whole:
        staging = 'tiles'
      else:
        staging = (f'planes{1 << ppb_log2}' if tiles_y == 1 else 'bands') + '/' + form(run_vec)
      return kernel, staging, 'k4' if k4 else 'loop'
  return 'direct', None, None


# ---- reference and bound ----------------------------------------------------------------------------------------------
def define(x, k, params, dtype=torch.float64):
  """The definition: x [major, H, W, minor], k [kh, kw] -> [major, oh, ow, minor], in `dtype` torch on the CPU."""
  major, H, W, minor, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1 = params
  x, k = x.to(dtype), k.to(dtype)
  planes = x.permute(0, 3, 1, 2).reshape(major * minor, 1, H, W)
  u = torch.zeros(major * minor, 1, H * uy, W * ux, dtype=dtype)
  u[:, :, ::uy, ::ux] = planes
  u = F.pad(u, (px0, px1, py0, py1))
  y = F.conv2d(u, torch.flip(k, (0, 1)).view(1, 1, kh, kw), stride=(dy, dx))
  assert tuple(y.shape[2:]) == out_hw(params), (y.shape, params)
  return y.reshape(major, minor, y.shape[2], y.shape[3]).permute(0, 2, 3, 1).contiguous()


def want_and_mag(x, k, old, beta, params):
  """float64 result and B, the sum of the absolute terms of every output element."""
  want, mag = define(x, k, params), define(x.abs(), k.abs(), params)
  if beta != 0.0:
    want, mag = want + beta * old.double(), mag + (beta * old.double()).abs()
  return want, mag


def bound(want, mag, params, dtype=torch.float32):
  """The per-element bound of the module text, as a float64 tensor."""
  n = params[4] * params[5] + 2
  if dtype == torch.float64:
    return n * 2.0 ** -53 * mag
  if dtype == torch.float16:
    return 2.0 ** -11 * want.abs() + n * U * mag + 2.0 ** -25
  return n * U * mag


def check(got, want, bnd, what, show=False):
  """|got - want| <= bnd element by element, no NaN; returns (and prints with show) the worst error / bound."""
  ratio = within(got, want, bnd / U, 1.0, what)
  if show:
    print(f'  {what}: worst error / bound = {ratio:.3g}')
  return ratio


_INPUTS = {}


def inputs(case):
  """(x [major, H, W, minor], taps [kh, kw], old [major, oh, ow, minor]) in fp32, cached and never modified."""
  if case.name not in _INPUTS:
    major, H, W, minor, kh, kw = case.params[:6]
    g = torch.Generator().manual_seed(4000 + IDS.index(case.name))
    e = torch.linspace(-2.0, 2.0, major) if major > 1 else torch.zeros(1)
    order = [i // 2 if i % 2 == 0 else major - 1 - i // 2 for i in range(major)]      # neighbours far apart
    scale = (10.0 ** e[order]).view(major, 1, 1, 1)
    x = torch.randn(major, H, W, minor, generator=g) * scale
    k = torch.randn(kh, kw, generator=g)
    oh, ow = out_hw(case.params)
    old = torch.randn(major, oh, ow, minor, generator=g) * scale
    _INPUTS[case.name] = (x, k, old)
  return _INPUTS[case.name]


# ---- guarded buffers ------------------------------------------------------------------------------------------------
class Guarded:
  """`t` inside a byte buffer on `dev`: GUARD_BYTES of `fill` bytes, (4 more for one_in,) the payload, GUARD_BYTES again."""

  def __init__(self, t, dev, one_in, fill):
    nbytes = t.numel() * t.element_size()
    self.off = GUARD_BYTES + (4 if one_in else 0)
    total = (self.off + nbytes + GUARD_BYTES + 15) & ~15
    host = torch.full((total,), fill, dtype=torch.uint8)
    host[self.off:self.off + nbytes] = t.contiguous().view(-1).view(torch.uint8)
    self.host = host
    self.buf = place(host, dev)
    self.end = self.off + nbytes
    self.t = self.buf[self.off:self.end].view(t.dtype).view(t.shape)
    assert self.t.is_contiguous() and self.t.data_ptr() % 16 == (4 if one_in else 0)

  def guards_intact(self):
    now = self.buf.cpu()
    return torch.equal(now[:self.off], self.host[:self.off]) and torch.equal(now[self.end:], self.host[self.end:])


def guarded_in(t, dev, one_in=False):
  """An operand between NaN guards (0xFF bytes are a NaN in half, float and double)."""
  g = Guarded(t, dev, one_in, 0xFF)
  return g.t


def guarded_out(t, dev, one_in=False):
  return Guarded(t, dev, one_in, SENTINEL)


ENTRY = {torch.float32: 'upfirdn2d_f32', torch.float16: 'upfirdn2d_f16', torch.float64: 'upfirdn2d_f64'}


def run(lib, case, beta, dtype=torch.float32):
  """One guarded launch of `case`: stk_upfirdn2d_acc_f32 for beta != 0, the plain entry of `dtype` otherwise.  Returns
  (result on the CPU, float64 reference, B); the guards are asserted here."""
  from _util import dev_of
  x, k, old = inputs(case)
  x, k = x.to(dtype), k.to(dtype)
  d = dev_of(lib)
  start = old if beta != 0.0 else torch.full_like(old, float('nan'))
  out = guarded_out(start.to(dtype), d, case.one_in)
  a, b = guarded_in(x, d, case.one_in), guarded_in(k, d, case.one_in)
  stream = torch.cuda.current_stream().cuda_stream if lib.is_device else 0
  args = (a.data_ptr(), b.data_ptr(), out.t.data_ptr())
  if beta != 0.0:
    assert dtype == torch.float32
    lib.upfirdn2d_acc_f32(*args, float(beta), *case.params, stream)
  else:
    getattr(lib, ENTRY[dtype])(*args, *case.params, stream)
  if lib.is_device:
    torch.cuda.synchronize()
  assert out.guards_intact(), f'{case.name}: a write outside the output'
  want, mag = want_and_mag(x, k, old, beta, case.params)           # from the rounded inputs and taps
  return out.t.cpu().clone(), want, mag


# ---- extent rule ----------------------------------------------------------------------------------------------------
# a negative numerator and an even `down`: C's division gives -1 / 2 + 1 = 1 row (column), floor division none
EXTENT_CASES = [
  ('rows', (2, 1, 8, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)),
  ('cols', (2, 8, 1, 1, 4, 4, 1, 1, 2, 2, 1, 1, 1, 1)),
]
STK_EINVAL = -1


def extent_refused(lib, params, dtype):
  """The entry of `dtype` on an empty output extent: returns (status, whether the 4 KB guarded buffer it was given as
  output is untouched).  The row a truncating division would write is 2 x 4 elements: it cannot leave the buffer."""
  from _util import dev_of
  d = dev_of(lib)
  assert out_hw(params) is None
  g = torch.Generator().manual_seed(7)
  x = torch.randn(params[0], params[1], params[2], params[3], generator=g).to(dtype)
  k = torch.randn(params[4], params[5], generator=g).to(dtype)
  out = guarded_out(torch.full((512,), float('nan')).to(dtype), d)
  a, b = guarded_in(x, d), guarded_in(k, d)
  stream = torch.cuda.current_stream().cuda_stream if lib.is_device else 0
  rc = getattr(lib, ENTRY[dtype]).raw(a.data_ptr(), b.data_ptr(), out.t.data_ptr(), *params, stream)
  rc_acc = None
  if dtype == torch.float32:
    rc_acc = lib.upfirdn2d_acc_f32.raw(a.data_ptr(), b.data_ptr(), out.t.data_ptr(), 0.5, *params, stream)
  if lib.is_device:
    torch.cuda.synchronize()
  untouched = torch.equal(out.buf.cpu(), out.host)
  return rc, rc_acc, untouched
