"""What a step launches, read from the plan alone: a recording proxy of a loaded library and a dry runtime that walks a
finalized graph over fake base addresses exactly as engine/executor.py does (Executor.program, Executor._runtime and the
executor's forward / backward loops), so the launch sequence of every mode can be pinned on a machine without a GPU
(tests/test_launch_trace.py, tests/golden/launch_trace.json).

The GPU tests that look at the launches of a real step use the same proxy in its executing form (`execute=True`)."""
import hashlib

import numpy as np

SWITCHES = ('STK_PLANES', 'STK_PLANES_WGRAD', 'STK_X_RECORDS', 'STK_SHARED_DY', 'STK_RES_VIA', 'STK_DY_PRODUCER',
            'STK_GN_FOLD_BATCH', 'STK_WGRAD_STREAM')
TINY = ('vp', 'rve', 've', 'wide', 'wide_mh', 've_cat', 'vp_ff')
SHIPPED = ('cifar10_ddpmpp_nll_st', 'imagenet32_ddpmpp_st', 'celeba_uncsnpp_st', 'celebahq_uncsnpp_st')
FULL_TEXT = ('wide',)             # models whose traces the fixture keeps as text (the others: count and digest); `wide`
                                  # alone is 400 KB of text in all modes, and it is the family that takes every fused path

# fake handles and base addresses: distinct, far apart, 256-byte aligned
MAIN, SIDE = 0x51 << 32, 0x52 << 32
BASES = {k: (i + 1) << 40 for i, k in enumerate(
  ('act', 'gact', 'param', 'gparam', 'const', 'ws', 'ws2', 'wp', 'pl', 'dypl', 'gnpart', 'gn_table', 'seed_dev'))}
SEED = 0x5EED


def is_launch(L, name):
  """Is entry `name` (without the stk_ prefix) of engine/lib.py a launch, i.e. does it take a stream as its last argument?
  (The pointer and the stream type are the same ctypes class, so the queries that end in a pointer are told apart by
  L._NO_CHECK, the entries of every header that are bound unchecked.)"""
  full = 'stk_' + name
  for table in (L.SIGNATURES, *(h.table for h in L.OPTIONAL_HEADERS)):
    row = table.get(full)
    if row is not None:
      return bool(row) and row[-1] is L.S and full not in L._NO_CHECK
  return False                     # not an entry of the C ABI at all (a helper of StkLib)


class LibProxy:
  """A loaded StkLib seen through a recorder.  Attributes that are not callable pass through; a launch is appended to
  `log` as (entry name, arguments) and, unless `execute`, NOT forwarded; every other entry is a query and is forwarded."""

  def __init__(self, L, lib, log=None, execute=False):
    self._L, self._lib, self._execute = L, lib, execute
    self.log = [] if log is None else log

  def __getattr__(self, name):
    f = getattr(self._lib, name)
    if not callable(f):
      return f
    if not is_launch(self._L, name):
      return f

    def call(*a):
      self.log.append((name, a))
      if self._execute:
        return f(*a)
    call.__name__ = name
    return call


class _Side:
  """engine/executor.SideStream without a device: hands out the fake side handle and logs the fork / join."""

  def __init__(self, log):
    self.log, self.last = log, None

  def begin(self):
    self.log.append(('<fork>', ()))
    return SIDE

  def end(self):
    self.last = True
    return self.last

  def join(self):
    if self.last is not None:
      self.log.append(('<join>', ()))
      self.last = None


class _Prof:
  """engine/profile.KernelTimer without events: the label rides on the launch it brackets."""

  def __init__(self, log):
    self.log = log

  def launch(self, kind, flops, fn, args):
    n = len(self.log)
    fn(*args)
    assert len(self.log) == n + 1, f'{kind}: a timed call is one launch'
    self.log[n] = self.log[n] + ((kind, flops),)


def _fmt(a):
  if a is None:
    return '-'
  if isinstance(a, (bool, int, np.integer)):
    a = int(a)
    return hex(a) if a >= 1 << 32 else str(a)
  if isinstance(a, (float, np.floating)):
    return repr(float(a))
  raise TypeError(f'launch argument {a!r}')


def lines(log):
  out = []
  for name, args, *label in log:
    s = ' '.join([name] + [_fmt(a) for a in args])
    if label:
      s += f' # {label[0][0]} {_fmt(label[0][1])}'
    out.append(s)
  return out


def digest(text_lines):
  return hashlib.sha256('\n'.join(text_lines).encode()).hexdigest()


def build_model(st, name):
  """(network on the CPU, its FlatParams, batch, height, width) of a tiny family or a shipped config."""
  import torch
  from _model_util import tiny_config
  if name in TINY:
    cfg, B = tiny_config(st, name), 4
  else:
    cfg = getattr(st.configs, name)()
    cfg.device = torch.device('cpu')
    B = cfg.training.batch_size
  net = st.models.ncsnpp.NCSNpp(cfg, st.sde_lib.get_sde(cfg, None))
  flat = st.engine.flat.FlatParams(list(net.parameters()), 'cpu', groups=net._flat_groups())
  return net, flat, B, cfg.data.image_size, cfg.data.image_size


def modes(lib):
  """(mode name, precision, with_backward, side, prof, param_grads) of every mode traced on `lib`."""
  out = [('fwd.fp32', 'fp32', False, False, False, True)]
  if lib.has_fp16:
    out.append(('fwd.fp16', 'fp16', False, False, False, True))
  precisions = ['fp32'] + (['fp16-train'] if lib.has_fp16 and lib.has_fp16_train else [])
  for precision in precisions:
    for pg in (True, False):
      if lib.is_device:            # the executor gives a host backend no side stream (Executor._runtime)
        out.append((f'side.{precision}.pg{int(pg)}', precision, True, True, False, pg))
      out.append((f'prof.{precision}.pg{int(pg)}', precision, True, False, True, pg))
  return out


def trace(st, model, lib, precision='fp32', with_backward=True, side=False, prof=False, param_grads=True):
  """The launch log of one evaluation of `model` = (net, flat, B, H, W) on `lib`: forward, and with `with_backward` the
  backward behind it.  Returns (log, side stream attached?)."""
  import os
  G, L = st.engine.graph, st.engine.lib
  net, flat, B, H, W = model
  log = []
  proxy = LibProxy(L, lib, log)
  g = G.Graph(flat, proxy)                                   # Executor.program
  g.precision = precision
  g.finalize(net._emit(g, B, H, W, False), proxy)
  rt = G.Runtime(proxy, MAIN, BASES['act'], BASES['gact'], BASES['param'], BASES['gparam'], BASES['const'],
                 BASES['ws'], g.ws_bytes, with_backward, SEED, BASES['seed_dev'])
  rt.with_backward = with_backward                           # Executor._runtime
  rt.f16 = precision in ('fp16', 'fp16-train')
  rt.f16_bwd = precision == 'fp16-train'
  rt.param_grads = param_grads
  if prof:
    rt.prof = _Prof(log)
  if lib.is_device and any(off is not None for op in g.ops if isinstance(op, G.Conv) for off in op.wp_off):
    rt.wp = BASES['wp']
  if g.pl_bytes + g.dypl_bytes > 0:
    rt.pl, rt.dypl = BASES['pl'], BASES['dypl']
    if (side and with_backward and os.environ.get('STK_WGRAD_STREAM', '1') != '0' and lib.is_device and g.own_dypl):
      rt.side, rt.ws2 = _Side(log), BASES['ws2']
  if with_backward and g.gn_folds:
    rt.gnpart, rt.gn_table = BASES['gnpart'], BASES['gn_table']
    rt.gn_maxc = max(ch for *_, ch in g.gn_folds)
  for op in g.ops:
    op.forward(rt)
  if with_backward:
    log.append(('<backward>', ()))
    for op in reversed(g.ops):
      op.backward(rt)
    rt.flush_folds()
    rt.join_side()
  return log, rt.side is not None


def cases(st, libs):
  """Every (key, model name, library name, mode tuple, switch) of the fixture; `libs` = {'product': lib, 'checker': lib}."""
  for model in TINY + SHIPPED:
    for lname, lib in libs.items():
      for mode in modes(lib):
        yield f'{model}/{lname}/{mode[0]}', model, lname, mode, None
  for switch in SWITCHES:
    for lname, lib in libs.items():
      for mode in modes(lib):
        yield f'wide/{lname}/{mode[0]}/{switch}=0', 'wide', lname, mode, switch


def record(st, libs, environ):
  """The whole fixture: key -> {launches, side (was the side stream attached?), sha256[, text]}.  `environ` (os.environ or a stand-in) has the eight switches
  removed and the one under test set while a case is traced."""
  out, models = {}, {}
  saved = {k: environ.pop(k) for k in SWITCHES if k in environ}
  try:
    for key, model, lname, mode, switch in cases(st, libs):
      if model not in models:
        models.clear()                                       # one network in memory at a time
        models[model] = build_model(st, model)
      if switch:
        environ[switch] = '0'
      try:
        log, has_side = trace(st, models[model], libs[lname], *mode[1:])
      finally:
        if switch:
          del environ[switch]
      text = lines(log)
      out[key] = {'launches': sum(1 for n, *_ in log if not n.startswith('<')), 'side': has_side, 'sha256': digest(text)}
      if model in FULL_TEXT and switch is None and mode[-1]:   # (param_grads=False launches a subset of the same lines)
        out[key]['text'] = text
  finally:
    environ.update(saved)
  return out
