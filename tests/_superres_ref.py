"""The float64 restatement of include/stk_superres.h that the super-resolution tests compare with, and the magnitude B of
their rounding bound.  Tensors are float64 on the host: x [N,C,H,W]; low, z [N,C,H/r,W/r]; a, s [N]."""
import torch
import torch.nn.functional as F

# d of csrc/superres.hip's header comment: the additions on the longest path from an element of x to its block sum,
# (r - 1) down the rows + log2 r over the columns.  Never more than P - 1 = r^2 - 1.
DEPTH = {2: 2, 4: 5, 8: 10, 16: 19}


def block_mean(x, r):
  return F.avg_pool2d(x, r)


def upsample(v, r):
  """Each value of [N,C,H/r,W/r] on the r x r pixels of its block."""
  return v.repeat_interleave(r, dim=2).repeat_interleave(r, dim=3)


def _wide(v):
  return v[:, None, None, None]


def restate(x, low, z, a, s, r):
  """The header's formulas -> (x_out, x_mean)."""
  m_x = block_mean(x, r)
  mean = _wide(a) * low
  known = mean if z is None else mean + _wide(s) / r * z
  return x + upsample(known - m_x, r), x + upsample(mean - m_x, r)


def magnitude(x, low, z, a, s, r):
  """B of the bound k 2^-24 B: |x| + blockmean|x| + |a||low| + |s||z| / r, broadcast to the pixels."""
  b = block_mean(x.abs(), r) + _wide(a.abs()) * low.abs()
  if z is not None:
    b = b + _wide(s.abs()) / r * z.abs()
  return x.abs() + upsample(b, r)
