"""The streaming attention kernels (csrc/attention_long.hip) on every width, length edge and launch form: the case table,
the launch rule of `launch_c` / `nw_dq` / `tpad` / `mh_short` restated, the operands of each input family, the placements
as flat buffers and the guarded launch sequence (tests/test_gpu_attention_long_forms.py on the HIP library,
tests/test_attention_long_cases_cpu.py without a GPU).  The bounds and the numpy model are tests/_attn_long_ref.py; the
float64 reference, the placements' helpers and the classic input families are those of the short table
(tests/_attn_ref.py, tests/_attn_cases.py).

Entries.  'long': stk_attention_long_fwd_f32 / _bwd_f32, one head, every T.  'mh': stk_attention_mh_fwd_f32 / _bwd_f32, which
reach these kernels only for T > 256 (mh_short); with heads == 1 that is the same launch sequence as the long entry and the
GPU test asserts equal bits.

The launch rule (launch_rule()).  Tp = T rounded up to 128; a workgroup owns 16 NW positions: 128 queries in the forward
(NW_FWD = 8), 128 queries in DQ up to d = 192 and 64 from d = 224 on (nw_dq), 64 keys in DKV (NW_DKV = 4); the grids are
B heads Tp / tile.  stage_cf / stage_pf move N = 8 d 16-byte pieces a chunk with NT = 64 NW threads: their guarded branch
(N % NT != 0) runs at d = 96, 160, 224 on the forward, d = 96, 160 on DQ (d = 224 has NT = 256) and never on DKV; at d = 32
on the forward and DQ N < NT (the guarded branch as well, with half of the threads idle).  With T = 132, Tp = 256: the
upper waves of the second forward tile, and the last DQ / DKV workgroup of 64, own dead positions only.

Placements, beta, scale as in _attn_cases.py.  null: the gradients passed as NULL, a tuple of indices into (dq, dk, dv);
(1, 2) launches no DKV kernel.  Input families: randn, decades, apart, negative, offset, coherent and the floor cases
'floor peaked' / 'floor unattended' are _attn_cases._inputs's.  The streaming ones (d = 64 or 32, at least four chunks):
  rising        the score rises by 2 a chunk along the keys: every chunk raises every row's maximum (alpha < 1 every time).
  last chunk    the maximum sits in the last (partial) chunk, 30 above the rest: everything before is rescaled by e^-30.
  first chunk   the maximum sits in the first chunk: alpha = 1 ever after, later chunks add terms of e^-30.
  ds up keys    p, and so |ds|, grows 4x a chunk along the keys: DQ's column scale drops at every chunk.
  ds up queries d_o grows 4x a chunk along the queries: DKV's column scale drops at every chunk.
  ds falls      p falls 2^-4 a chunk along the keys and d_o 2^-4 a chunk along the queries: later terms sit under the scale
                in use, down to 2^-16 of it.
  peaked        one-hot rows: query t looks along one channel, scale s = 200 k[j(t), t'].  dq and dk are held like every
                output: ds = p (dp - delta) cancels on the peak, and E_dp + E_delta in the bound carry that.
  tiny do       d_o = 2^-100 randn: the columns' ds scales reach 2^115 and beyond, and s_k sig passes 2^127.
Floor cases (FLOOR_CASES: the floor is more than half the bound somewhere, and the model shows a quarter of it there):
  floor peaked, floor unattended   as in the short table: the probabilities' split at 2^13 in o and in dv.
  floor ds keys     the column floor of dq: the keys 64 .. carry p = 0.33 2^-38, v = 0 (ds = -p delta, one sign) and ARE
                    identical, so their split residuals add up; channel 0 of the attended keys is zero, so dq[0, t] is
                    what the unattended keys contribute.
  floor ds queries  the column floor of dk: the queries 64 .. are one query with d_o 2^-33 of the others'; channel 0 of
                    the other queries is zero.  (The short table's 'floor ds row' could not reach its floor because a
                    64-wide tile shares the scale and the small row's residuals cancel; identical rows do not cancel.)
"""
import collections
import functools

import numpy as np

import _attn_cases as ac
import _attn_long_ref as al
import _attn_ref as ar

STK_OK, STK_EINVAL, STK_EUNSUPPORTED = ac.STK_OK, ac.STK_EINVAL, ac.STK_EUNSUPPORTED
TRIPLE, NPART, PLACES = ac.TRIPLE, ac.NPART, ac.PLACES
KC, TPAD, NW_FWD, NW_DKV, DQ_4_WAVES_FROM, MH_SHORT_T = 32, 128, 8, 4, 224, 256
GRAD = ('dq', 'dk', 'dv')

Case = collections.namedtuple('Case', 'name entry B C heads T place beta scale null fam')


def _c(entry, B, C, heads, T, place, beta='zero', scale='d', null=(), fam='randn'):
  name = (f'{entry}_B{B}C{C}h{heads}T{T}_{place}_{beta}_s{scale}' + ('' if not null else '_null' + ''.join(GRAD[i][1] for i in null))
          + '_' + fam.replace(' ', '-'))
  return Case(name, entry, B, C, heads, T, place, beta, scale, tuple(null), fam)


CASES = [
  # ---- the long entries: every T edge, every width --------------------------------------------------------------------------
  _c('long', 1, 32, 1, 4, 'separate', fam='negative'),                          # one chunk, 4 live keys; forward grid 1
  _c('long', 3, 64, 1, 28, 'stacked', 'triple', 0.37, fam='negative'),          # grid 3
  _c('long', 2, 96, 1, 32, 'padded', fam='decades'),
  _c('long', 7, 160, 1, 36, 'mixed-a', 'triple', fam='negative'),               # grid 7; the second chunk holds 4 keys
  _c('long', 2, 224, 1, 60, 'mixed-b', null=(0,), fam='negative'),
  _c('long', 2, 256, 1, 64, 'padded', 'triple', fam='apart'),
  _c('long', 9, 64, 1, 68, 'separate', scale=0.37, null=(1,), fam='negative'),  # grid 9; DKV grid 18
  _c('long', 2, 128, 1, 124, 'stacked', null=(2,), fam='negative'),
  _c('long', 2, 192, 1, 128, 'mixed-a', 'triple', fam='offset'),
  _c('long', 5, 96, 1, 132, 'padded', 'triple', fam='negative'),                # grids 10, 10, 20: above 8, no multiple of 8
  _c('long', 2, 160, 1, 252, 'mixed-b', scale=0.37, fam='negative'),
  _c('long', 1, 224, 1, 260, 'separate', 'triple', fam='negative'),
  _c('long', 1, 64, 1, 388, 'stacked', null=(1, 2), fam='negative'),            # no DKV launch
  _c('long', 1, 32, 1, 516, 'mixed-a', fam='negative'),                         # 17 chunks
  _c('long', 2, 256, 1, 132, 'separate', null=(0, 1)),                          # 4 DQ waves; dv alone
  _c('long', 3, 32, 1, 260, 'padded', 'triple', 0.37),
  # ---- the streaming families -------------------------------------------------------------------------------------------------
  _c('long', 2, 64, 1, 128, 'separate', fam='rising'),
  _c('long', 2, 64, 1, 124, 'separate', fam='last chunk'),
  _c('long', 2, 64, 1, 132, 'separate', fam='first chunk'),
  _c('long', 2, 64, 1, 128, 'separate', fam='ds up keys'),
  _c('long', 2, 64, 1, 128, 'separate', fam='ds up queries'),
  _c('long', 2, 64, 1, 132, 'separate', fam='ds falls'),
  _c('long', 2, 32, 1, 128, 'separate', fam='peaked'),
  _c('long', 2, 64, 1, 128, 'separate', fam='tiny do'),
  _c('mh', 1, 64, 2, 260, 'separate', fam='tiny do'),
  # ---- the floor cases and the coherent split ---------------------------------------------------------------------------------
  _c('long', 2, 32, 1, 28, 'separate', fam='floor peaked'),
  _c('long', 1, 32, 1, 128, 'separate', fam='floor unattended'),
  _c('long', 1, 32, 1, 128, 'separate', fam='floor ds keys'),
  _c('long', 1, 32, 1, 128, 'separate', fam='floor ds queries'),
  _c('long', 2, 64, 1, 64, 'separate', fam='coherent'),
  # ---- the MH entries on the streaming path: every head width at T = 260 ----------------------------------------------------
  _c('mh', 1, 64, 2, 260, 'separate', scale=0.37, fam='negative'),              # d = 32
  _c('mh', 2, 96, 3, 260, 'stacked', 'triple'),                                 # d = 32, odd head count, B = 2
  _c('mh', 1, 128, 2, 260, 'padded', scale=0.37, null=(0,), fam='decades'),     # d = 64
  _c('mh', 1, 192, 2, 260, 'mixed-a', 'triple', null=(1,), fam='negative'),     # d = 96
  _c('mh', 1, 256, 2, 260, 'mixed-b', null=(2,)),                               # d = 128
  _c('mh', 1, 320, 2, 260, 'padded', 'triple', fam='offset'),                   # d = 160
  _c('mh', 1, 448, 2, 260, 'stacked', fam='apart'),                             # d = 224
  _c('mh', 1, 512, 2, 260, 'separate', 'triple', fam='negative'),               # d = 256, C = 512
  _c('mh', 2, 128, 4, 388, 'mixed-a', fam='negative'),
  _c('mh', 1, 128, 1, 260, 'separate', 'triple'),                               # one head: the long entry's bits
]
IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FLOOR_CASES = {'floor peaked': ('o',), 'floor unattended': ('dv',), 'floor ds keys': ('dq',), 'floor ds queries': ('dk',)}
T_VALUES = (4, 28, 32, 36, 60, 64, 68, 124, 128, 132, 252, 260, 388, 516)
D_VALUES = (32, 64, 96, 128, 160, 192, 224, 256)
MH_D_VALUES = (32, 64, 96, 128, 160, 224, 256)
STREAM_FAMILIES = ('rising', 'last chunk', 'first chunk', 'ds up keys', 'ds up queries', 'ds falls', 'peaked', 'tiny do')


# ---- the launch rule, restated -------------------------------------------------------------------------------------------------
def scale_of(c):
  return ac.scale_of(c)


def tpad(T):
  return -(-T // TPAD) * TPAD


def launch_rule(B, heads, d, T):
  """{kernel: (tile, grid, ragged staging, N < NT)} of 'fwd', 'dq', 'dkv' for B heads pairs of d channels."""
  out = {}
  for kern, nw in (('fwd', NW_FWD), ('dq', 4 if d >= DQ_4_WAVES_FROM else 8), ('dkv', NW_DKV)):
    n, nt = 8 * d, 64 * nw
    out[kern] = (16 * nw, B * heads * (tpad(T) // (16 * nw)), n % nt != 0, n < nt)
  return out


def streaming(c):
  """The MH entry runs the short kernels up to T = 256."""
  return c.entry == 'long' or c.T > MH_SHORT_T


def forms(c):
  """Everything case c reaches (strings, the vocabulary of REQUIRED)."""
  d = c.C // c.heads
  ent = 'long' if c.entry == 'long' else ('mh heads' if c.heads > 1 else 'mh one head')
  rule = launch_rule(c.B, c.heads, d, c.T)
  f = {ent, f'{ent} T {c.T}', f'{ent} d {d}', f'{c.entry} {c.place}', f'{c.entry} beta {c.beta}', f'{c.entry} scale {c.scale}',
       f'fam {c.fam}', f'fwd grid {rule["fwd"][1]}', f'dq waves {rule["dq"][0] // 16}'}
  runs = {'fwd': True, 'dq': 0 not in c.null, 'dkv': not {1, 2} <= set(c.null)}
  for kern, (tile, grid, ragged, short) in rule.items():
    if not runs[kern]:
      continue
    if ragged:
      f.add(f'ragged {kern} d {d}')
    if short:
      f.add(f'{kern} N < NT')
    if grid > 8 and grid % 8:
      f.add(f'{kern} grid above 8, no multiple of 8')
    if kern == 'dkv' and grid > 16:
      f.add('dkv grid above 16')
  if c.null:
    f.add(f'{c.entry} null {c.null}')
  if c.C == 512 and c.heads == 2:
    f.add('C 512')
  if c.fam == 'negative':
    f.add(f'negative T {c.T}')
  return f


def _required():
  R = {'long', 'mh heads', 'mh one head', 'mh one head T 260', 'mh heads T 260', 'mh heads T 388', 'C 512'}
  R |= {f'long T {T}' for T in T_VALUES} | {f'long d {d}' for d in D_VALUES} | {f'mh heads d {d}' for d in MH_D_VALUES}
  R |= {f'ragged fwd d {d}' for d in (96, 160, 224)} | {f'ragged dq d {d}' for d in (96, 160)} | {'fwd N < NT', 'dq N < NT'}
  R |= {'dq waves 4', 'dq waves 8'} | {f'fwd grid {g}' for g in (1, 3, 7, 9)} | {'dkv grid above 16'}
  R |= {f'{k} grid above 8, no multiple of 8' for k in ('fwd', 'dq', 'dkv')}
  for ent in ('long', 'mh'):
    R |= {f'{ent} {p}' for p in PLACES} | {f'{ent} beta zero', f'{ent} beta triple', f'{ent} scale d', f'{ent} scale 0.37'}
    R |= {f'{ent} null {(i,)}' for i in range(3)}
  R |= {'long null (1, 2)', 'long null (0, 1)'}
  R |= {f'negative T {T}' for T in T_VALUES if T % KC}
  R |= {f'fam {f}' for f in ('randn', 'decades', 'apart', 'negative', 'offset', 'coherent') + STREAM_FAMILIES + tuple(FLOOR_CASES)}
  return R


REQUIRED = _required()


# ---- operands ------------------------------------------------------------------------------------------------------------------
def _inputs(c):
  seed = 5100 + IDS.index(c.name)
  fam = c.fam
  if fam not in STREAM_FAMILIES and fam not in ('floor ds keys', 'floor ds queries'):
    return ac._inputs(c, seed)
  if fam in ('tiny do', 'floor ds queries'):
    t = ac._inputs(c._replace(fam='randn'), seed)
    q, k, v, do = (t[n].astype(np.float64) for n in ('q', 'k', 'v', 'do'))
    if fam == 'tiny do':
      do = do * 2.0 ** -100
    else:
      q[:, :, 64:], do[:, :, 64:] = q[:, :, 64:65], 2.0 ** -33 * do[:, :, 64:65]
      q[:, 0, :64] = 0.0
  else:
    B, C, T, d = c.B, c.C, c.T, c.C // c.heads
    assert c.heads == 1
    scale = scale_of(c)
    rng = np.random.default_rng(seed)
    rn = lambda *s: rng.standard_normal(s)
    u = rn(C)
    u = (u / np.linalg.norm(u))[None, :, None]
    chunk = np.arange(T) // KC
    pos = np.arange(T, dtype=np.float64)
    a = 1.0 / scale                                                             # q = a u: scale s = u . k
    v, do = rn(B, C, T), rn(B, C, T)
    if fam == 'rising':
      q, k = a * u + 0.05 * rn(B, C, T), u * (pos / 16.0) + 0.05 * rn(B, C, T)
    elif fam in ('last chunk', 'first chunk'):
      q, k = a * u + 0.02 * rn(B, C, T), 0.05 * rn(B, C, T)
      where = slice(T - 3, T) if fam == 'last chunk' else slice(0, 3)
      k[:, :, where] += 30.0 * u
    elif fam == 'ds up keys':
      q, k = a * u + 0.01 * rn(B, C, T), u * (pos * np.log(4.0) / KC) + 0.01 * rn(B, C, T)
    elif fam == 'ds up queries':
      q, k = rn(B, C, T), rn(B, C, T)
      do = do * 4.0 ** chunk
    elif fam == 'ds falls':
      q, k = a * u + 0.01 * rn(B, C, T), -u * (pos * np.log(16.0) / KC) + 0.01 * rn(B, C, T)
      do = do * 16.0 ** -chunk
    elif fam == 'peaked':
      j = rng.integers(0, C, (B, T))
      q = np.zeros((B, C, T))
      np.put_along_axis(q, j[:, None, :], 1.0 / scale, 1)
      k = 200.0 * rn(B, C, T)
    elif fam == 'floor ds keys':
      u0 = rng.choice([-1.0, 1.0], d)[None, :, None]
      a = ((38 * np.log(2.0) - np.log(0.33) - np.log(64.0)) / (scale * d)) ** 0.5
      sg = 0.1 / (scale * a * d ** 0.5)
      q, k = a * u0 + sg * rn(B, C, T), sg * rn(B, C, T)
      k[:, :, 64:] = -a * u0
      k[:, 0, :64] = 0.0
      v, do = np.abs(v), np.abs(do)
      v[:, :, 64:] = 0.0
    else:
      raise ValueError(fam)
  t = {n: np.ascontiguousarray(x, dtype=np.float32) for n, x in (('q', q), ('k', k), ('v', v), ('do', do))}
  t['g0'] = [np.full(t['q'].shape, np.nan, np.float32)] * 3
  assert c.beta == 'zero'
  return t


@functools.lru_cache(maxsize=4)
def inputs(name):
  """The float32 operands of a case (cached, never modified): q, k, v, do of [B, C, T] and g0, the three initial gradients."""
  return _inputs(BY_NAME[name])


def betas(c):
  return ac.betas(c)


@functools.lru_cache(maxsize=2)
def reference(name):
  """(want, bnd, ref): the float64 outputs of a case as the launch leaves them (beta g0 added), the bounds of
  tests/_attn_long_ref.py and the bare reference (_attn_ref.reference) with its 'aux' quantities, computed once."""
  c, t = BY_NAME[name], inputs(name)
  ref = ar.reference(t['q'], t['k'], t['v'], t['do'], c.heads, scale_of(c))
  bnd = al.bounds(ref, t['q'], t['k'], t['v'], t['do'], c.heads, scale_of(c), betas(c), t['g0'])
  want = {n: ref[n] for n in ar.OUTPUTS}
  for i, n in enumerate(GRAD):
    if betas(c)[i] != 0.0:
      want[n] = betas(c)[i] * t['g0'][i].astype(np.float64) + ref[n]
  return want, bnd, ref


def checked(c):
  """The outputs a case is held to: a NULL gradient is compared with its initial bits instead."""
  return tuple(n for n in ar.OUTPUTS if n not in GRAD or GRAD.index(n) not in c.null)


# ---- placements: flat buffers (the helpers of _attn_cases.py on this table's operands) ---------------------------------------------
def layout(c):
  """_attn_cases.layout for a case of this table."""
  t = inputs(c.name)
  ct = c.C * c.T
  bs, gs, qst, gst = ac.strides(c)
  sign = lambda i: np.float32((2.0 if i % 2 == 0 else -2.0) * np.abs(t['qkv'[i]]).max())
  ins = ac._flat([t['q'], t['k'], t['v']], c.B, ct, bs, qst, sign)
  grads = ac._flat(t['g0'], c.B, ct, gs, gst, lambda i: ac.GAP_SENTINEL)
  written = [np.zeros(f.shape, bool) for f in grads[0]]
  for i, (bi, off) in enumerate(grads[1]):
    if i not in c.null:
      for b in range(c.B):
        written[bi][off + b * gs:off + b * gs + ct] = True
  return {'in': ins, 'grad': grads, 'written': written, 'bs': bs, 'gs': gs}


def run_model(c, mutant=None):
  """The numpy model on the buffers of case c, read and written at the strides the host code passes on.  mutant: one of
  _attn_long_ref.MUTANTS or 'gradients at the qkv stride'."""
  t, L = inputs(c.name), layout(c)
  B, C, T = c.B, c.C, c.T
  ct, shape = C * T, (B, C, T)
  q, k, v = (ac.gather(L['in'][0][bi], off, B, ct, L['bs'], shape) for bi, off in L['in'][1])
  out = al.model(q, k, v, t['do'], c.heads, scale_of(c), betas(c), t['g0'], None if mutant == 'gradients at the qkv stride' else mutant)
  ws = L['bs'] if mutant == 'gradients at the qkv stride' else L['gs']
  bufs = [f.copy() for f in L['grad'][0]]
  for i, n in enumerate(GRAD):
    bi, off = L['grad'][1][i]
    if i in c.null:
      continue
    for b in range(B):
      seg = bufs[bi][off + b * ws:off + b * ws + ct]
      seg[:] = out[n][b].reshape(-1)[:seg.size]
  for i, n in enumerate(GRAD):
    bi, off = L['grad'][1][i]
    out[n] = ac.gather(bufs[bi], off, B, ct, L['gs'], shape)
  return out


# ---- the launch sequence ---------------------------------------------------------------------------------------------------------
def ws_bytes_of(lib, c, entry=None):
  entry = entry or c.entry
  return int(lib.attention_long_ws_bytes(c.B, c.C, c.T) if entry == 'long' else lib.attention_mh_ws_bytes(c.B, c.C, c.T, c.heads))


def run(lib, c, fill=0xFF, entry=None, dev='cuda'):
  """One forward and one backward of case c through the C ABI (entry: the case's, or 'long' for a one-head MH case) on fresh
  guarded buffers, the workspace of exactly ws_bytes() bytes filled with `fill` bytes (fp16 NaN) before the forward and again
  before the backward -> the outputs and 'rec' as numpy arrays.  Asserted here: the guards of every buffer, every element
  of the gradient buffers outside the images (gaps, a NULL gradient's slice), the operands' bits."""
  import torch
  from _stream_util import Guarded
  entry = entry or c.entry
  assert fill & 0x7C == 0x7C and fill & 0x03, 'the fill has to read as an fp16 NaN'
  t, L = inputs(c.name), layout(c)
  B, C, T, H = c.B, c.C, c.T, c.heads
  nan = lambda *s: np.full(s, np.nan, np.float32)
  gin = [Guarded(f, dev) for f in L['in'][0]]
  ggr = [Guarded(f, dev) for f in L['grad'][0]]
  gdo = Guarded(t['do'], dev)
  nws = ws_bytes_of(lib, c, entry)
  assert nws > 0 and nws % 16 == 0, (c.name, nws)
  G = {'o': Guarded(nan(B, C, T), dev), 'lse': Guarded(nan(B, H, T), dev), 'delta': Guarded(nan(B, H, T), dev),
       'rec': Guarded(nan(4 * NPART), dev), 'ws': Guarded(np.full(nws, fill, np.uint8).view(np.float32), dev)}
  ws_bits = G['ws'].view.view(torch.int32)
  fill32 = int(np.full(4, fill, np.uint8).view(np.int32)[0])
  ptr = lambda g, off: g.view.data_ptr() + 4 * off
  ins = [ptr(gin[bi], off) for bi, off in L['in'][1]]
  outs = [None if i in c.null else ptr(ggr[bi], off) for i, (bi, off) in enumerate(L['grad'][1])]
  bq, bk, bv = betas(c)
  scale = scale_of(c)
  stream = torch.cuda.current_stream().cuda_stream
  o, lse, delta, rec, ws = (G[n].view.data_ptr() for n in ('o', 'lse', 'delta', 'rec', 'ws'))
  assert ws % 16 == 0 and bool((ws_bits == fill32).all())
  if entry == 'long':
    assert H == 1 and lib.attention_long_ok(B, C, T) == 1, c.name
    lib.attention_long_fwd_f32(ins[0], ins[1], ins[2], L['bs'], o, lse, rec, B, C, T, scale, ws, nws, stream)
    ws_bits.fill_(fill32)
    lib.attention_long_bwd_f32(ins[0], ins[1], ins[2], L['bs'], o, gdo.view.data_ptr(), lse, rec, delta, outs[0], bq, outs[1], bk,
                               outs[2], bv, L['gs'], B, C, T, scale, ws, nws, stream)
  else:
    assert lib.attention_mh_ok(B, C, T, H) == 1 and streaming(c), c.name
    lib.attention_mh_fwd_f32(ins[0], ins[1], ins[2], L['bs'], o, lse, rec, B, C, T, H, scale, ws, nws, stream)
    ws_bits.fill_(fill32)
    lib.attention_mh_bwd_f32(ins[0], ins[1], ins[2], L['bs'], o, gdo.view.data_ptr(), lse, rec, delta, outs[0], bq, outs[1], bk,
                             outs[2], bv, L['gs'], B, C, T, H, scale, ws, nws, stream)
  torch.cuda.synchronize()
  for n, g in list(G.items()) + [(f'in{i}', g) for i, g in enumerate(gin)] + [(f'grad{i}', g) for i, g in enumerate(ggr)] + [('do', gdo)]:
    g.check(f'{c.name} {n}')
  bits = lambda a: np.ascontiguousarray(a).view(np.int32)
  for i, g in enumerate(gin):
    assert np.array_equal(bits(g.view.cpu().numpy()), bits(L['in'][0][i])), f'{c.name}: operand buffer {i} was written'
  assert np.array_equal(bits(gdo.view.cpu().numpy()), bits(t['do'])), f'{c.name}: do was written'
  got = {n: G[n].view.cpu().numpy() for n in ('o', 'lse', 'delta', 'rec')}
  flat = [g.view.cpu().numpy() for g in ggr]
  for i, f in enumerate(flat):
    keep = ~L['written'][i]
    assert np.array_equal(bits(f)[keep], bits(L['grad'][0][i])[keep]), \
        f'{c.name}: gradient buffer {i} was written outside its images (a gap, or the slice of a NULL gradient)'
  for i, n in enumerate(GRAD):
    bi, off = L['grad'][1][i]
    got[n] = ac.gather(flat[bi], off, B, C * T, L['gs'], (B, C, T))
  return got
