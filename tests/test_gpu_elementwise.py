"""Every entry of csrc/elementwise.hip through the C ABI on the device, element by element against the float64 restatements of
tests/_ew_ref.py: |got - want| <= k u B (u = 2^-24, B the entry's expression on absolute values, k derived there, never
measured on a kernel), bit for bit where an entry does no arithmetic.  The cases are tests/_ew_cases.py's: both launch forms
of launch_ew (16-byte and scalar, the scalar one by length and by a misaligned operand at a length divisible by 4), lengths
above the grid cap on each form, beta in {0 (NaN-prefilled output), 0.5, 1}, the optional operands absent, activations at
+-0, subnormals, the exp overflow and underflow thresholds and +-3e38, row scales from 0.01 to 348.  Every operand sits
between sentinels that must come back untouched.  tests/test_ew_cases_cpu.py holds the checker and a float32 restatement to
the same bounds without a GPU; STK_SELFCHECK=1 runs this file against the checker.

One line per test and launch form, `ew-accuracy ...`, gives the worst err / (u B) beside its k (profiles/elementwise_accuracy.txt).
"""
import pytest

import _ew_cases as ec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('group', ec.GROUP_IDS)
def test_entry(hip_lib, group):
  entry, size = ec.GROUPS[ec.GROUP_IDS.index(group)]
  worst = {}
  for case in ec.group_cases(entry, size):
    if entry == 'fourier_embedding_bwd' and not hip_lib.has_blocks:
      assert not hip_lib.is_device, 'the product library lacks include/stk_blocks.h'
      got = ec.restatement(entry, case.p)                # self-check on the checker, which lacks this entry
    else:
      got = ec.run(hip_lib, case)
      ec.check_null_matches_full(hip_lib, case)
    units, k = ec.check(case, got)
    form = case.form + ('+stride' if case.strided else '')
    worst[form] = max(worst.get(form, (0.0, k, '')), (units, k, ec.case_name(case)))
  for form, (units, k, name) in worst.items():
    print(f'ew-accuracy {entry:24s} {form:14s} worst {units:8.3f} k {k:6g}   ({name})')
