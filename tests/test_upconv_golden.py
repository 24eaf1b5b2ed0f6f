"""tests/golden/model_vp_ddpm_fir.npz is what tools/make_golden_upconv.py computes from the live reference (with this
repository's restatement standing in for its broken upsample_conv_2d): regenerated where the reference is present and
compared array by array; the reference never travels, so elsewhere this skips."""
import os
import sys

import numpy as np
import pytest

import refimport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'model_vp_ddpm_fir.npz')


def test_fixture_is_data_within_the_size_limit():
  assert os.path.getsize(GOLDEN) < 1 << 20
  with np.load(GOLDEN) as f:
    assert all(f[k].dtype.kind in 'fiu' for k in f.files)
    assert any(k.startswith('sd.') and 'Conv2d_0.weight' in k for k in f.files)      # the Upsample's fused convolution


@pytest.mark.skipif(not refimport.available(), reason='the reference is not on this machine')
def test_fixture_is_what_the_reference_computes():
  if os.path.join(ROOT, 'tools') not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
  import make_golden_upconv as mk
  got = mk.generate()
  with np.load(GOLDEN) as f:
    assert sorted(f.files) == sorted(got)
    for k in f.files:
      want = f[k]
      assert got[k].shape == want.shape and got[k].dtype == want.dtype, k
      scale = max(float(np.abs(want).max()), 1e-30)
      # the same float32 program on the same machine class: equal up to the thread count's summation order
      assert float(np.abs(got[k].astype(np.float64) - want).max()) <= 1e-5 * scale + 1e-9, k
