"""The launch sequence of a step, pinned: every C-ABI launch with every argument (and its profiler label), for the tiny
model families, the shipped configs and the debugging switches, read from the plan on fake addresses -- no launch is
executed, so this runs without a GPU (tests/_launch_trace.py).  The numeric tests catch a wrong fusion; this catches a lost
one (an extra pass over dy computes the same numbers) and any drift of the two-stream plan.

tests/golden/launch_trace.json is rewritten by `python tools/make_golden.py launch_trace`: do that only for a change that
MEANS to alter what is launched, and read the diff of the `text` entries."""
import difflib
import json
import os

import pytest

import _launch_trace as lt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'launch_trace.json')
REWRITE = 'python tools/make_golden.py launch_trace'

with open(GOLDEN) as _f:
  FIXTURE = json.load(_f)
_MODELS = {}


@pytest.fixture(scope='module')
def libs(st, ref_lib):
  try:
    return {'product': st.engine.lib.load(), 'checker': ref_lib}
  except st.engine.lib.StkMissingError:
    pytest.fail('libstk.so is not built (run __graft_entry__.build())')


def _model(st, name):
  if name not in _MODELS:
    _MODELS.clear()                                          # one network in memory at a time (cases are grouped by model)
    _MODELS[name] = lt.build_model(st, name)
  return _MODELS[name]


def test_fixture_lists_every_case(st, libs):
  assert sorted(FIXTURE) == sorted(key for key, *_ in lt.cases(st, libs)), f'rewrite the fixture: {REWRITE}'


@pytest.mark.parametrize('key', list(FIXTURE))
def test_launch_trace(st, libs, monkeypatch, tmp_path, key):
  model, lname, mode, *switch = key.split('/')
  for name in lt.SWITCHES:
    monkeypatch.delenv(name, raising=False)
  if switch:
    monkeypatch.setenv(*switch[0].split('='))
  lib = libs[lname]
  _, precision, with_backward, side, prof, param_grads = next(m for m in lt.modes(lib) if m[0] == mode)
  log, has_side = lt.trace(st, _model(st, model), lib, precision, with_backward, side, prof, param_grads)
  text = lt.lines(log)
  launches = [(n, a) for n, a, *_ in log if not n.startswith('<')]
  want = FIXTURE[key]
  if lt.digest(text) != want['sha256'] or len(launches) != want['launches']:
    got = tmp_path / 'trace.txt'
    got.write_text('\n'.join(text) + '\n')
    diff = '\n'.join(difflib.unified_diff(want.get('text', []), text, 'golden', 'traced', lineterm='', n=1))
    pytest.fail(f'{key}: {len(launches)} launches (golden: {want["launches"]}), trace written to {got}; if the change is '
                f'meant, rewrite the fixture with `{REWRITE}`\n' + (diff if 'text' in want else ''), pytrace=False)
  # what a digest cannot say
  assert launches, 'an empty trace pins nothing'
  # (the executor attaches the side stream to a context with a planes arena only -- the 8-channel tiny families have none --
  # and not under STK_WGRAD_STREAM=0)
  assert has_side == want['side'] and (has_side or not side or switch or model not in ('wide',) + lt.SHIPPED)
  on_side = {n for n, a in launches if a[-1] == lt.SIDE}
  wgrads = [(n, a) for n, a in launches if n.startswith('conv2d_wgrad_')]
  if has_side:       # two streams: every weight gradient on the side stream, and nothing else
    assert all(a[-1] == lt.SIDE for _, a in wgrads) and all(n.startswith('conv2d_wgrad_') for n in on_side), on_side
    assert [n for n, *_ in log].count('<fork>') == len(wgrads)
  else:
    assert not on_side and all(a[-1] == lt.MAIN for _, a in launches)
  if precision == 'fp32':
    assert not [n for n, _ in launches if n.endswith('_f16x1')]
  if not param_grads:
    assert not wgrads and not [n for n, _ in launches if n == 'gn_param_grad_batch']
  if prof:
    assert any(len(e) == 3 for e in log), 'the profiler labels are part of the trace'
