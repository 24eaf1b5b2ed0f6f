"""The three entries of include/stk_cond.h restated in float64 on the host, with the magnitudes their rounding bounds are
stated against.  Operands are fp32 tensors (their values are exact in float64); nothing here rounds to fp32.

  class_row       idx(b): the index when it is an integer in [0, C], else the null row C
  embed_fwd       y = t + table[idx]                      magnitude |t| + |e|                       (one rounding)
  embed_bwd_gt    gt' = gy (beta 0) or gt + gy (beta 1)   magnitude |gt| + |gy|                     (one rounding)
  embed_bwd_table gtable[c] += sum of gy[b], idx(b) == c  magnitude |g0| + sum |gy|, count n_c      (n_c roundings)
  cfg_combine     out = c + w (c - u)                     magnitude |c| + |w| (|c| + |u|)           (three roundings)
"""
import torch


def class_row(idx, C):
  """[B] long: the table row of every sample.  idx: [B] fp32-encoded indices (any float value)."""
  f = idx.double()
  ok = torch.isfinite(f) & (f >= 0) & (f <= C) & (f == torch.trunc(f))
  return torch.where(ok, f, torch.full_like(f, float(C))).long()


def embed_fwd(t, table, idx):
  """(y, magnitude) in float64."""
  C = table.shape[0] - 1
  e = table.double()[class_row(idx, C)]
  return t.double() + e, t.double().abs() + e.abs()


def embed_bwd_gt(gy, gt, beta):
  """(gt', magnitude) in float64; beta in {0, 1}."""
  if beta == 0:
    return gy.double(), gy.double().abs()
  return gt.double() + gy.double(), gt.double().abs() + gy.double().abs()


def embed_bwd_table(gy, idx, gtable):
  """(gtable', magnitude, count) in float64: count[c] = n_c, the samples of row c; rows with n_c = 0 keep their value."""
  C = gtable.shape[0] - 1
  rows = class_row(idx, C)
  out, mag = gtable.double().clone(), gtable.double().abs().clone()
  out.index_add_(0, rows, gy.double())
  mag.index_add_(0, rows, gy.double().abs())
  count = torch.bincount(rows, minlength=C + 1)
  return out, mag, count


def cfg_combine(c, u, w):
  """(out, magnitude) in float64; w a Python float that is exact in fp32."""
  c, u = c.double(), u.double()
  return c + w * (c - u), c.abs() + abs(w) * (c.abs() + u.abs())
