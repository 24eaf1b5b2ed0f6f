"""The bias-gradient family and the row softmax of csrc/reduce_optim.hip on every branch of their kernels and host wrappers
(tests/test_reduce_cases_cpu.py: the checker against float64; tests/test_gpu_reduce.py: the HIP library against the checker).

Reference: the checker's double-accumulating restatement (oracle/stk_ref.c), itself held to float64 torch sums in the CPU
half.  Bounds, u = 2^-24, (roundings in the chain) x 2 x u x (sum of the absolute terms), written next to each kernel form:

  rows[n, c] = alpha * sum_hw dy          k_row = chain + 6 (wave reduction) + 1 (alpha) [+ 3: the four waves of
                                          rowsum_block_kernel], chain = the longest `s +=` run of one lane:
                                            float4 rows   ceil(HW / 4 / 64) + 2   (+ 2: the tree inside one float4)
                                            scalar rows   ceil(HW / 64)
                                            block kernel  ceil(HW / 4 / 256) + 2
                                          |err| <= 2 k_row u |alpha| sum_hw |dy|
  dbias[c] += alpha * sum_{n, hw} dy      fused kernel: k_row + 2 ceil(N / 32) (rows of one wave) + 16 (the waves) + 1 (+=)
                                          rowsum + colsum_acc_kernel: k_row + ceil(N / 8) + 8 + 1
                                          |err| <= 2 k u (|alpha| sum_{n, hw} |dy| + |dbias_0|)
  amax[c] = max |dy[:, c, :]|             exact, zeros up to 256 entries; HW >= 4096 (stk_amax_partial_f32): any partition
                                          of the tensor, so only the maximum of the record is fixed
  res = alpha * dy + rbeta * res          3 roundings: |err| <= 6 u (|alpha dy| + |rbeta res_0|); rbeta == 0: res_0 is not read
                                          (it holds NaN in those cases)
  softmax y = exp(x s - mx) / sum         argument: fl(fl(x s) - mx) is off by at most 3 a u, a = max_j |x_j s| OF THE ROW (the
                                          denominator carries the other elements' arguments, so the row maximum and not the
                                          element's own |x| is the rigorous form); expf within 1 ulp = 2 u, in the numerator and
                                          in the denominator; the sum (chain = ceil(cols / 64), + 6), 1 / s, the product:
                                          |err| <= 2 (4 + chain + 8) u y + 2 * 6 a u y;   |sum_j y_j - 1| <= cols u
  softmax dx = s y (dy - d), d = sum y dy the difference, two products: 3; d: chain + 6 roundings relative to sum |y dy|:
                                          |err| <= 2 u s |y| (3 (|dy| + |d|) + (chain + 6) sum_j |y_j dy_j|)

Host dispatch restated (`branch`; H = HW):
  stk_bias_grad_f32         dbias and H < 4096 -> bias_grad_kernel<0,0>; else rows go to dtemb (or ws): H >= 4096, H % 4 == 0
                            and dy aligned -> rowsum_block_kernel, else rowsum_kernel (float4 rows iff H % 4 == 0 and the row
                            is aligned); then colsum_acc_kernel if dbias
  stk_bias_grad_amax_f32    H < 4096 -> bias_grad_kernel<1,0>; else stk_bias_grad_f32 + stk_amax_partial_f32
  stk_bias_grad_amax_res_f32  H < 4096 -> bias_grad_kernel<1,1>; else stk_axpby_f32 + the amax entry
  stk_bias_grad_amax_dual_f32 H < 4096 only -> bias_grad_kernel<1,0> with dbias2 / amax2
  bias_grad_kernel: float4 rows iff H % 4 == 0 and dy (and res) are 16-byte aligned.  Wave w takes rows n = w, w + 32, ... and
  n2 = n + 16 with it: `rows2` says whether n2 < N held for none / some / all of the (wave, iteration) pairs, `iters` is
  ceil(N / 32).

Case table: BIAS_CASES and SOFTMAX_CASES below, one row per case with its branch label.
"""
import numpy as np
import torch

from _util import call, dev_of

U = 2.0 ** -24

# name, entry, N, C, HW, options, branch
#   entry: plain / amax / res / dual;   options: dtemb (rows wanted), nodbias, mis_dy, mis_res, beta (rbeta = 0.5)
BIAS_CASES = []
_ROWS2 = {1: ('none', 1), 16: ('none', 1), 17: ('some', 1), 32: ('all', 1), 33: ('some', 2), 48: ('some', 2), 128: ('all', 4)}
_T = {'plain': '0,0', 'amax': '1,0', 'res': '1,1', 'dual': '1,0'}
for _N, (_r2, _it) in _ROWS2.items():
  for _e in ('plain', 'amax', 'res', 'dual'):
    BIAS_CASES.append((f'{_e}_N{_N}', _e, _N, 6, 64, 'dtemb beta' if _N % 2 else '',
                       f'bias_grad_kernel<{_T[_e]}>:vec rows2={_r2} iters={_it}'))
for _e in ('plain', 'amax', 'res', 'dual'):
  BIAS_CASES += [
    (f'{_e}_hw25', _e, 17, 5, 25, 'dtemb', f'bias_grad_kernel<{_T[_e]}>:scalar rows2=some iters=1'),
    (f'{_e}_hw81', _e, 33, 3, 81, 'beta', f'bias_grad_kernel<{_T[_e]}>:scalar rows2=some iters=2'),
    (f'{_e}_mis_dy', _e, 17, 5, 64, 'dtemb mis_dy', f'bias_grad_kernel<{_T[_e]}>:scalar rows2=some iters=1'),
  ]
BIAS_CASES += [
  ('res_mis_res', 'res', 17, 5, 64, 'dtemb mis_res beta', 'bias_grad_kernel<1,1>:scalar rows2=some iters=1'),
  ('res_mis_res_beta0', 'res', 16, 5, 64, 'mis_res', 'bias_grad_kernel<1,1>:scalar rows2=none iters=1'),
  ('plain_C33', 'plain', 9, 33, 4096, '', 'rowsum_block_kernel+colsum_acc_kernel'),
  ('plain_C1', 'plain', 3, 1, 4096, '', 'rowsum_block_kernel+colsum_acc_kernel'),
  ('plain_C1_rows', 'plain', 1, 1, 64, 'dtemb nodbias', 'rowsum_kernel:vec'),
  ('rows_only_vec', 'plain', 3, 5, 64, 'dtemb nodbias', 'rowsum_kernel:vec'),
  ('rows_only_hw25', 'plain', 3, 5, 25, 'dtemb nodbias', 'rowsum_kernel:scalar'),
  ('rows_only_mis', 'plain', 3, 5, 64, 'dtemb nodbias mis_dy', 'rowsum_kernel:scalar'),
  ('long_aligned', 'plain', 3, 10, 4096, 'dtemb', 'rowsum_block_kernel+colsum_acc_kernel'),
  ('long_aligned_rows', 'plain', 2, 3, 8192, 'dtemb nodbias', 'rowsum_block_kernel'),
  ('long_4100', 'plain', 2, 3, 4100, 'dtemb', 'rowsum_block_kernel+colsum_acc_kernel'),
  ('long_mis_dy', 'plain', 3, 10, 4096, 'dtemb mis_dy', 'rowsum_kernel:scalar+colsum_acc_kernel'),
  ('long_4097', 'plain', 2, 3, 4097, '', 'rowsum_kernel:scalar+colsum_acc_kernel'),
  ('amax_long', 'amax', 2, 5, 4096, 'dtemb', 'rowsum_block_kernel+colsum_acc_kernel+amax_partial'),
  ('amax_long_mis', 'amax', 2, 5, 4096, 'mis_dy', 'rowsum_kernel:scalar+colsum_acc_kernel+amax_partial'),
  ('res_long', 'res', 2, 5, 4096, 'dtemb beta', 'axpby+rowsum_block_kernel+colsum_acc_kernel+amax_partial'),
]
BIAS_IDS = [c[0] for c in BIAS_CASES]
assert len(set(BIAS_IDS)) == len(BIAS_IDS)

BIAS_KERNELS = {'bias_grad_kernel<0,0>', 'bias_grad_kernel<1,0>', 'bias_grad_kernel<1,1>', 'rowsum_kernel',
                'rowsum_block_kernel', 'colsum_acc_kernel'}


def _rows2(N):
  pairs = [(w + 32 * j) + 16 < N for w in range(16) for j in range(-(-N // 32)) if w + 32 * j < N]
  return 'all' if all(pairs) else 'some' if any(pairs) else 'none'


def branch(case, dy, res):
  """The kernels the host wrapper launches for this case, from the shape and the addresses actually passed."""
  name, entry, N, C, HW, opt, _ = case
  al = dy.data_ptr() % 16 == 0
  dbias = 'nodbias' not in opt

  def plain():
    if dbias and HW < 4096:
      return None
    if HW >= 4096 and HW % 4 == 0 and al:
      k = 'rowsum_block_kernel'
    else:
      k = 'rowsum_kernel:' + ('vec' if HW % 4 == 0 and al else 'scalar')
    return k + ('+colsum_acc_kernel' if dbias else '')

  if HW < 4096 and (entry != 'plain' or dbias):
    vec = HW % 4 == 0 and al and (entry != 'res' or res.data_ptr() % 16 == 0)
    return f"bias_grad_kernel<{_T[entry]}>:{'vec' if vec else 'scalar'} rows2={_rows2(N)} iters={-(-N // 32)}"
  assert entry != 'dual', 'stk_bias_grad_amax_dual_f32 refuses HW >= 4096'
  return ('axpby+' if entry == 'res' else '') + plain() + ('+amax_partial' if entry != 'plain' else '')


def _place(t, d, mis):
  if not mis:
    out = t.to(d).contiguous().clone()
    assert out.data_ptr() % 16 == 0
    return out
  buf = torch.empty(t.numel() + 1, device=d)
  assert buf.data_ptr() % 16 == 0
  buf[1:] = t.reshape(-1).to(d)
  v = buf[1:].view(t.shape)
  assert v.data_ptr() % 16 == 4 and v.is_contiguous()
  return v


def bias_inputs(case):
  name, entry, N, C, HW, opt, _ = case
  gen = torch.Generator().manual_seed(900 + N * 7 + C * 3 + HW)
  inp = {'dy': torch.randn(N, C, HW, generator=gen), 'db0': torch.randn(C, generator=gen),
         'db20': torch.randn(C, generator=gen), 'alpha': 0.5 if 'beta' in opt else 1.0,
         'rbeta': 0.5 if 'beta' in opt else 0.0}
  inp['res0'] = torch.randn(N, C, HW, generator=gen) if 'beta' in opt else torch.full((N, C, HW), float('nan'))
  return inp


def bias_run(lib, case, inp):
  """Call the entry; outputs as CPU tensors and the branch reached.  Everything the entry must write starts as NaN."""
  name, entry, N, C, HW, opt, _ = case
  d = dev_of(lib)
  TS = C + 3                                                     # rows go into a wider [N, TS] tensor at column 2
  dy = _place(inp['dy'], d, 'mis_dy' in opt)
  res = _place(inp['res0'], d, 'mis_res' in opt) if entry == 'res' else None
  reached = branch(case, dy, res)
  dt = torch.full((N, TS), float('nan'), device=d) if 'dtemb' in opt else None
  db = inp['db0'].to(d).clone() if 'nodbias' not in opt else None
  ws = torch.full((N * C,), float('nan'), device=d)
  dtp = dt.data_ptr() + 2 * 4 if dt is not None else None
  out = {}
  if entry == 'plain':
    call(lib, 'bias_grad_f32', dy, N, C, HW, inp['alpha'], dtp, TS, db, ws)
  else:
    amax = torch.full((256,), float('nan'), device=d)
    if entry == 'amax':
      call(lib, 'bias_grad_amax_f32', dy, N, C, HW, inp['alpha'], dtp, TS, db, amax, ws)
    elif entry == 'res':
      call(lib, 'bias_grad_amax_res_f32', dy, N, C, HW, inp['alpha'], dtp, TS, db, amax, res, inp['rbeta'], ws)
      out['res'] = res.cpu().clone()
    else:
      db2, amax2 = inp['db20'].to(d).clone(), torch.full((256,), float('nan'), device=d)
      call(lib, 'bias_grad_amax_dual_f32', dy, N, C, HW, inp['alpha'], dtp, TS, db, amax, db2, amax2, ws)
      out['dbias2'], out['amax2'] = db2.cpu(), amax2.cpu()
    out['amax'] = amax.cpu()
  if lib.is_device:
    torch.cuda.synchronize()
  if dt is not None:
    out['rows'] = dt.cpu()[:, 2:2 + C].clone()
    rest = torch.cat([dt.cpu()[:, :2], dt.cpu()[:, 2 + C:]], 1)
    assert bool(torch.isnan(rest).all()), f'{name}: columns outside [2, 2 + C) of dtemb were written'
  if db is not None:
    out['dbias'] = db.cpu()
  assert torch.equal(dy.cpu(), inp['dy']), f'{name}: dy was modified'
  return out, reached


def bias_float64(case, inp):
  """The same quantities in float64 torch, with the sums of absolute terms the bounds need."""
  name, entry, N, C, HW, opt, _ = case
  dy, a = inp['dy'].double(), inp['alpha']
  r = {'rows': a * dy.sum(2), 'rows_abs': abs(a) * dy.abs().sum(2)}
  r['dbias'] = inp['db0'].double() + a * dy.sum((0, 2))
  r['dbias2'] = inp['db20'].double() + a * dy.sum((0, 2))
  r['dbias_abs'] = abs(a) * dy.abs().sum((0, 2)) + inp['db0'].double().abs()
  r['dbias2_abs'] = abs(a) * dy.abs().sum((0, 2)) + inp['db20'].double().abs()
  r['amax'] = inp['dy'].abs().amax((0, 2))
  if inp['rbeta'] != 0.0:
    r['res'] = a * dy + inp['rbeta'] * inp['res0'].double()
    r['res_abs'] = (a * dy).abs() + (inp['rbeta'] * inp['res0'].double()).abs()
  else:
    r['res'], r['res_abs'] = a * dy, (a * dy).abs()
  return r


def _chains(case, reached):
  name, entry, N, C, HW, opt, _ = case
  if 'rowsum_block_kernel' in reached:
    k_row = -(-(HW // 4) // 256) + 2 + 6 + 3 + 1
  elif ':vec' in reached:
    k_row = -(-(HW // 4) // 64) + 2 + 6 + 1
  else:
    k_row = -(-HW // 64) + 6 + 1
  k_db = k_row + (-(-N // 8) + 8 + 1 if 'colsum' in reached else 2 * -(-N // 32) + 16 + 1)
  return k_row, k_db


def _worst(err, bound):
  err, bound = err.double(), bound.double()
  r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
  r[~torch.isfinite(err)] = float('inf')
  return float(r.max()) if r.numel() else 0.0


def bias_figures(case, got, ref, f64, reached, slack=2.0):
  """worst |got - ref| / bound per output; ref: the checker's outputs (or float64 in the checker's own test)."""
  name, entry, N, C, HW, opt, _ = case
  k_row, k_db = _chains(case, reached)
  fig = {}
  if 'rows' in got:
    fig['rows'] = _worst((got['rows'].double() - ref['rows'].double()).abs(), slack * k_row * U * f64['rows_abs'])
  for k in ('dbias', 'dbias2'):
    if k in got:
      fig[k] = _worst((got[k].double() - ref[k].double()).abs(), slack * k_db * U * f64[k + '_abs'])
  for k in ('amax', 'amax2'):
    if k in got:
      a = got[k]
      if HW < 4096:
        ok = torch.equal(a[:C], f64['amax']) and float(a[C:].abs().max() if C < 256 else 0.0) == 0.0
      else:
        ok = float(a.max()) == float(f64['amax'].max()) and float(a.min()) >= 0.0
      fig[k] = 0.0 if ok else float('inf')
  if 'res' in got:
    fig['res'] = _worst((got['res'].double() - ref['res'].double()).abs(), slack * 3 * U * f64['res_abs'])
  return fig


# ---- softmax -----------------------------------------------------------------------------------------------------------
SOFTMAX_SCALE = 0.0625
SOFTMAX_ROWS = 9                      # not a multiple of the 4 rows of one workgroup
# cols -> the branch: `s +=` iterations of the busiest lane of the one wave that owns a row
SOFTMAX_CASES = [(1, 'lane_iters=1 lanes=1'), (63, 'lane_iters=1 lanes=63'), (64, 'lane_iters=1 lanes=64'),
                 (65, 'lane_iters=2 lanes=64'), (1024, 'lane_iters=16 lanes=64')]


def softmax_branch(cols):
  return f'lane_iters={-(-cols // 64)} lanes={min(cols, 64)}'


def softmax_inputs(cols):
  """row 0: one logit 80 above the rest (after the scale); row 1: equal logits; the others 3 N(0,1)."""
  gen = torch.Generator().manual_seed(500 + cols)
  x = torch.randn(SOFTMAX_ROWS, cols, generator=gen) * 3
  x[0, cols // 2] += 80.0 / SOFTMAX_SCALE
  x[1] = 3.7
  return x, torch.randn(SOFTMAX_ROWS, cols, generator=gen)


def softmax_run(lib, x, dy):
  d = dev_of(lib)
  rows, cols = x.shape
  y = torch.full((rows, cols), float('nan'), device=d)
  call(lib, 'softmax_fwd_f32', x.to(d), y, rows, cols, SOFTMAX_SCALE)
  dx = dy.to(d).clone()
  call(lib, 'softmax_bwd_f32', y, dx, dx, rows, cols, SOFTMAX_SCALE)         # in place, as the attention op uses it
  if lib.is_device:
    torch.cuda.synchronize()
  return y.cpu(), dx.cpu()


def softmax_figures(x, dy, y, dx):
  """Figures of the forward against float64 softmax(x * scale) and of the backward against float64 from the library's y."""
  cols = x.shape[1]
  chain = -(-cols // 64)
  s = float(np.float32(SOFTMAX_SCALE))
  xs = x.double() * s
  y64 = torch.softmax(xs, 1)
  a = xs.abs().amax(1, keepdim=True)
  fig = {'y': _worst((y.double() - y64).abs(), (2 * (4 + chain + 8) * U + 12 * a * U) * y64),
         'row_sum': _worst((y.double().sum(1) - 1).abs(), torch.full((x.shape[0],), cols * U, dtype=torch.float64))}
  yd = y.double()
  dsum = (yd * dy.double()).sum(1, keepdim=True)
  dx64 = s * yd * (dy.double() - dsum)
  bound = 2 * U * s * yd.abs() * (3 * (dy.double().abs() + dsum.abs()) + (chain + 6) * (yd * dy.double()).abs().sum(1, keepdim=True))
  fig['dx'] = _worst((dx.double() - dx64).abs(), bound)
  return fig
