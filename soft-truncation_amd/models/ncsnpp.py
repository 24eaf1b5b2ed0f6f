"""NCSN++ / DDPM++ score network (reference: models/ncsnpp.py:34-432).

``NCSNpp(config, sde)`` builds the same flat ``all_modules`` list as the reference constructor
(:38-256) -- same order, same attribute names, same initialisers -- so ``state_dict`` keys and
shapes are identical (``all_modules.<i>.<Name>.weight`` ...).  ``forward(x, time_cond)`` has the
reference's signature and semantics (:258-432) but does not walk the modules eagerly: the walk
happens once per input signature in ``_emit`` and produces a planned graph that the HIP engine
executes (engine/graph.py, engine/executor.py).  There is no PyTorch/CPU execution path.
"""
import functools

import numpy as np
import torch
import torch.nn as nn

from . import layers, layerspp, utils
from ..engine import executor as _executor
from ..engine import graph as G
from ..engine import lib as _stk_lib
from ..engine.graph import SQRT2

ResnetBlockDDPM = layerspp.ResnetBlockDDPMpp
ResnetBlockBigGAN = layerspp.ResnetBlockBigGANpp
Combine = layerspp.Combine
conv3x3 = layerspp.conv3x3
conv1x1 = layerspp.conv1x1
get_act = layers.get_act
default_initializer = layers.default_init


def _gn(ch):
  return nn.GroupNorm(num_groups=min(ch // 4, 32), num_channels=ch, eps=1e-6)


class ClassTable(nn.Module):
  """The class rows of a class-conditional network: ``weight`` [C + 1, D], row C the null class, all zeros at first -- a
  fresh conditional network then computes what the unconditional one does, and an unconditional checkpoint loaded with
  ``strict=False`` is a warm start.  A holder of the parameter only: the rows are added inside the planned graph
  (engine.graph.ClassEmbedding)."""

  def __init__(self, num_classes, dim):
    super().__init__()
    self.weight = nn.Parameter(torch.zeros(num_classes + 1, dim))


class AugmentTable(nn.Module):
  """The augmentation embedding of a network trained under non-leaky augmentation (augment.py): ``weight`` [D, K], a linear
  map of the K augmentation labels into the time embedding without a bias, all zeros at first -- a fresh network then
  computes what the plain one does, and a plain checkpoint loaded with ``strict=False`` is a warm start.  A holder of the
  parameter only: the product is added inside the planned graph (engine.graph.AugmentEmbedding)."""

  def __init__(self, augment_dim, dim):
    super().__init__()
    self.weight = nn.Parameter(torch.zeros(dim, augment_dim))


@utils.register_model(name='ncsnpp')
class NCSNpp(nn.Module):
  """NCSN++ model."""

  def __init__(self, config, sde=None):
    super().__init__()
    self.sde = sde
    self.config = config
    self.act = act = get_act(config)
    self.act_code = layers.act_code(config)       # the kernels' code for it (include/stk.h STK_ACT_*)
    self.register_buffer('sigmas', torch.tensor(utils.get_sigmas(config)))

    m = config.model
    self.nf = nf = m.nf
    ch_mult = m.ch_mult
    self.num_res_blocks = num_res_blocks = m.num_res_blocks
    self.attn_resolutions = attn_resolutions = m.attn_resolutions
    self.attention = attention = m.attention
    dropout = m.dropout
    resamp_with_conv = m.resamp_with_conv
    self.num_resolutions = num_resolutions = len(ch_mult)
    self.input_size = config.data.image_size
    self.all_resolutions = all_resolutions = [config.data.image_size // (2 ** i) for i in range(num_resolutions)]

    self.conditional = conditional = m.conditional
    # class conditioning (absent from the reference): 0 = off, the network of the reference, key for key
    self.num_classes = num_classes = int(utils.config_option(config, 'model', 'num_classes', 0) or 0)
    if num_classes < 0 or (num_classes > 0 and not conditional):
      raise ValueError(f'config.model.num_classes = {num_classes} needs config.model.conditional (the class row is added to '
                       f'the time embedding) and must not be negative')
    # augmentation labels (absent from the reference): 0 = off, the network of the reference, key for key
    self.augment_dim = augment_dim = int(utils.config_option(config, 'model', 'augment_dim', 0) or 0)
    if augment_dim < 0 or (augment_dim > 0 and not conditional):
      raise ValueError(f'config.model.augment_dim = {augment_dim} needs config.model.conditional (the labels are mapped into '
                       f'the time embedding) and must not be negative')
    # scale-shift GroupNorm conditioning (absent from the reference): False = off, the network of the reference, key for key
    self.scale_shift_norm = ssn = bool(utils.config_option(config, 'model', 'scale_shift_norm', False))
    if ssn and not conditional:
      raise ValueError('config.model.scale_shift_norm needs config.model.conditional (the residual blocks modulate their '
                       'second GroupNorm by the time embedding)')
    fir = m.fir
    fir_kernel = m.fir_kernel
    self.skip_rescale = skip_rescale = m.skip_rescale
    self.resblock_type = resblock_type = m.resblock_type.lower()
    self.auxiliary_resblock = auxiliary_resblock = m.auxiliary_resblock
    self.progressive = progressive = m.progressive.lower()
    self.progressive_input = progressive_input = m.progressive_input.lower()
    self.embedding_type = embedding_type = m.embedding_type.lower()
    self.fourier_feature = fourier_feature = m.fourier_feature
    init_scale = m.init_scale
    assert progressive in ['none', 'output_skip', 'residual']
    assert progressive_input in ['none', 'input_skip', 'residual']
    assert embedding_type in ['fourier', 'positional']
    combine_method = m.progressive_combine.lower()
    combiner = functools.partial(Combine, method=combine_method)
    modules = []
    if embedding_type == 'fourier':
      assert config.training.continuous, "Fourier features are only used for continuous training."
      modules.append(layerspp.GaussianFourierProjection(embedding_size=nf, scale=m.fourier_scale))
      embed_dim = 2 * nf
      embed_dim_2 = nf
    else:
      embed_dim = m.embedding_dim if m.lsgm else nf
      embed_dim_2 = embed_dim
    self.embed_dim = embed_dim

    if conditional:
      for fin, fout in ((embed_dim, embed_dim_2 * 4), (embed_dim_2 * 4, embed_dim_2 * 4)):
        lin = nn.Linear(fin, fout)
        lin.weight.data = default_initializer()(lin.weight.shape)
        nn.init.zeros_(lin.bias)
        modules.append(lin)

    if fourier_feature:          # (models/ncsnpp.py:104-105: a parameter-free module, but it takes a slot of all_modules)
      modules.append(layerspp.FixedFouriereProjection())

    # attention heads (absent from the reference): model.num_heads = h, the same in every attention block, or
    # model.num_head_channels = d, h = C / d per block; neither: the single head of the reference
    num_heads = utils.config_option(config, 'model', 'num_heads', None)
    num_head_channels = utils.config_option(config, 'model', 'num_head_channels', None)
    if num_heads is not None and num_head_channels is not None:
      raise ValueError('config.model.num_heads and config.model.num_head_channels are both set: give one of them')
    if (num_heads is not None and int(num_heads) < 1) or (num_head_channels is not None and int(num_head_channels) < 1):
      raise ValueError(f'config.model.num_heads = {num_heads} / num_head_channels = {num_head_channels} must be positive')

    def AttnBlock(channels):
      if num_head_channels is not None:
        if channels % int(num_head_channels):
          raise ValueError(f'config.model.num_head_channels = {num_head_channels} does not divide the C = {channels} '
                           f'channels of attention block all_modules.{len(modules)}')
        h = channels // int(num_head_channels)
      else:
        h = 1 if num_heads is None else int(num_heads)
        if channels % h:
          raise ValueError(f'config.model.num_heads = {h} does not divide the C = {channels} channels of attention block '
                           f'all_modules.{len(modules)}')
      return layerspp.AttnBlockpp(channels=channels, init_scale=init_scale, skip_rescale=skip_rescale, num_heads=h)
    Upsample = functools.partial(layerspp.Upsample, with_conv=resamp_with_conv, fir=fir, fir_kernel=fir_kernel)
    if progressive == 'output_skip':
      self.pyramid_upsample = layerspp.Upsample(fir=fir, fir_kernel=fir_kernel, with_conv=False)
    elif progressive == 'residual':
      pyramid_upsample = functools.partial(layerspp.Upsample, fir=fir, fir_kernel=fir_kernel, with_conv=True)
    Downsample = functools.partial(layerspp.Downsample, with_conv=resamp_with_conv, fir=fir, fir_kernel=fir_kernel)
    if progressive_input == 'input_skip':
      self.pyramid_downsample = layerspp.Downsample(fir=fir, fir_kernel=fir_kernel, with_conv=False)
    elif progressive_input == 'residual':
      pyramid_downsample = functools.partial(layerspp.Downsample, fir=fir, fir_kernel=fir_kernel, with_conv=True)

    if resblock_type == 'ddpm':
      ResnetBlock = functools.partial(ResnetBlockDDPM, act=act, dropout=dropout, init_scale=init_scale,
                                      skip_rescale=skip_rescale, temb_dim=embed_dim_2 * 4, scale_shift_norm=ssn)
    elif resblock_type == 'biggan':
      ResnetBlock = functools.partial(ResnetBlockBigGAN, act=act, dropout=dropout, fir=fir,
                                      fir_kernel=fir_kernel, init_scale=init_scale,
                                      skip_rescale=skip_rescale, temb_dim=embed_dim_2 * 4, scale_shift_norm=ssn)
    else:
      raise ValueError(f'resblock type {resblock_type} unrecognized.')
    # ---- down path ----------------------------------------------------------------------------
    channels = config.data.num_channels
    if progressive_input != 'none':
      input_pyramid_ch = channels
    if fourier_feature and channels != 3:
      # the reference hard-codes the stem width as channels + 12 (= 4 x 3 sin / cos channels, models/ncsnpp.py:156-159) while its
      # FixedFouriereProjection emits 5 x channels: the two only agree for RGB, and the reference fails on its first forward
      raise ValueError(f'model.fourier_feature needs data.num_channels == 3 (stem of channels + 12 inputs), got {channels}')
    modules.append(conv3x3(channels + 12 if fourier_feature else channels, nf))      # (models/ncsnpp.py:156-159: 12 = 4 x 3 channels)
    hs_c = [nf]
    in_ch = nf
    for i_level in range(num_resolutions):
      for i_block in range(num_res_blocks):
        out_ch = nf * ch_mult[i_level]
        modules.append(ResnetBlock(in_ch=in_ch, out_ch=out_ch))
        in_ch = out_ch
        if all_resolutions[i_level] in attn_resolutions and attention:
          modules.append(AttnBlock(channels=in_ch))
        hs_c.append(in_ch)

      if i_level != num_resolutions - 1:
        if resblock_type == 'ddpm':
          modules.append(Downsample(in_ch=in_ch))
        elif auxiliary_resblock:
          modules.append(ResnetBlock(down=True, in_ch=in_ch))

        if progressive_input == 'input_skip':
          modules.append(combiner(dim1=input_pyramid_ch, dim2=in_ch))
          if combine_method == 'cat':
            in_ch *= 2
        elif progressive_input == 'residual':
          modules.append(pyramid_downsample(in_ch=input_pyramid_ch, out_ch=in_ch))
          input_pyramid_ch = in_ch

        if self.auxiliary_resblock:
          hs_c.append(in_ch)

    # ---- middle -------------------------------------------------------------------------------
    in_ch = hs_c[-1]
    if not auxiliary_resblock:
      hs_c.pop()
    modules.append(ResnetBlock(in_ch=in_ch))
    modules.append(AttnBlock(channels=in_ch))
    modules.append(ResnetBlock(in_ch=in_ch))
    pyramid_ch = 0

    # ---- up path ------------------------------------------------------------------------------
    num_res_for_upsampling = num_res_blocks + 1 if self.auxiliary_resblock else num_res_blocks
    for i_level in reversed(range(num_resolutions)):
      for i_block in range(num_res_for_upsampling):
        out_ch = nf * ch_mult[i_level]
        modules.append(ResnetBlock(in_ch=in_ch + hs_c.pop(), out_ch=out_ch))
        in_ch = out_ch

      if all_resolutions[i_level] in attn_resolutions and attention:
        modules.append(AttnBlock(channels=in_ch))

      if progressive != 'none':
        if i_level == num_resolutions - 1:
          if progressive == 'output_skip':
            modules.append(_gn(in_ch))
            modules.append(conv3x3(in_ch, channels, init_scale=init_scale))
            pyramid_ch = channels
          elif progressive == 'residual':
            modules.append(_gn(in_ch))
            modules.append(conv3x3(in_ch, in_ch, bias=True))
            pyramid_ch = in_ch
        else:
          if progressive == 'output_skip':
            modules.append(_gn(in_ch))
            modules.append(conv3x3(in_ch, channels, bias=True, init_scale=init_scale))
            pyramid_ch = channels
          elif progressive == 'residual':
            modules.append(pyramid_upsample(in_ch=pyramid_ch, out_ch=in_ch))
            pyramid_ch = in_ch

      if i_level != 0:
        if resblock_type == 'ddpm':
          modules.append(Upsample(in_ch=in_ch))
        elif auxiliary_resblock:
          modules.append(ResnetBlock(in_ch=in_ch, up=True))

    assert not hs_c

    if progressive != 'output_skip':
      modules.append(_gn(in_ch))
      modules.append(conv3x3(in_ch, channels, init_scale=init_scale))

    self.all_modules = nn.ModuleList(modules)
    if num_classes > 0:         # outside all_modules: the all_modules.<i>.* keys keep their indices
      self.class_emb = ClassTable(num_classes, embed_dim_2 * 4)
    if augment_dim > 0:         # outside all_modules too, after the class rows
      self.augment_emb = AugmentTable(augment_dim, embed_dim_2 * 4)
    self._class_ctx = None      # (classes, guidance, [classes; null]) in force: models.utils.class_condition
    self._aug_ctx = None        # the [B, K] augmentation labels in force: models.utils.augment_condition
    self._null_aug = {}
    self._cfg_rescale = 0.0     # ... and its guidance rescale, saved and restored with it
    self._rescale_ws = {}
    self._null_rows = {}
    self._engine = None
    self._backend = None

  # ------------------------------------------------------------------------------------------------
  # engine plumbing
  # ------------------------------------------------------------------------------------------------
  def set_backend(self, backend):
    """Test hook: run the planned graph on another implementation of include/stk.h."""
    self._backend = backend
    if self._engine is not None:
      self._engine.set_backend(backend)

  def engine(self):
    if self._engine is None:
      self._engine = _executor.Executor(self, backend=self._backend)
    return self._engine

  def _dense_blocks(self):
    return [mod for mod in self.all_modules if hasattr(mod, 'Dense_0')]

  def _flat_groups(self):
    groups = []
    dense = self._dense_blocks()
    if dense:
      groups += [[b.Dense_0.weight for b in dense], [b.Dense_0.bias for b in dense]]
    if self.num_classes:
      # beside the stacked projections at the bottom of the flat buffers: its gradient is among the last the backward
      # writes, as theirs are, so the buckets above become final as early as in the unconditional network
      groups.append([self.class_emb.weight])
    if self.augment_dim:
      groups.append([self.augment_emb.weight])      # beside the class rows, for the same reason
    for mod in self.modules():
      if isinstance(mod, layerspp.AttnBlockpp):
        ws, bs = mod.qkv_params()
        groups += [('cols', ws), bs]
    return tuple(groups)

  def _uses_dropout(self):
    return any(isinstance(mod, nn.Dropout) and mod.p > 0 for mod in self.modules())

  def null_classes(self, B, device):
    """[B] class indices that all name the null row, as the engine takes them (fp32-encoded)."""
    t = self._null_rows.get((B, device))
    if t is None:
      t = self._null_rows[(B, device)] = torch.full((B,), float(self.num_classes), dtype=torch.float32, device=device)
    return t

  def augment_labels(self, B, device):
    """The [B, K] augmentation labels the engine takes: those in force (models.utils.augment_condition), zeros -- a clean
    image, as in sampling -- with none; None for a network without the embedding."""
    if not self.augment_dim:
      return None
    if self._aug_ctx is not None:
      if self._aug_ctx.shape[0] != B:
        raise ValueError(f'augment_condition holds labels of {self._aug_ctx.shape[0]} samples, the batch evaluated has {B}')
      return self._aug_ctx
    t = self._null_aug.get((B, device))
    if t is None:
      t = self._null_aug[(B, device)] = torch.zeros(B, self.augment_dim, dtype=torch.float32, device=device)
    return t

  def forward(self, x, time_cond):
    """x [B,C,H,W] fp32, time_cond [B] fp32 -> [B,C,H,W] (models/ncsnpp.py:258-432).  A class-conditional network
    (config.model.num_classes > 0) takes the classes and the guidance weight in force (models.utils.class_condition): no
    classes, every sample on the null row; a guidance weight w != 0, ONE evaluation of [x; x] with classes [y; null] and
    out = c + w (c - u) of its halves -- by stk_cfg_combine_f32, or by torch operators under grad mode, where autograd
    has to see it.  A guidance rescale phi != 0 in force: out = (phi std(c) / std(g) + 1 - phi) g per sample instead, by
    stk_cfg_rescale_f32 (include/stk_guided.h), or by torch operators under grad mode."""
    B = x.shape[0]
    aug = self.augment_labels(B, x.device)
    if not self.num_classes:
      return self._forward(x, time_cond, None, aug)
    cls, w, both = self._class_ctx if self._class_ctx is not None else (self.null_classes(B, x.device), 0.0, None)
    if cls.shape[0] != B:
      raise ValueError(f'class_condition holds {cls.shape[0]} classes, the batch evaluated has {B} samples')
    if w == 0.0:
      return self._forward(x, time_cond, cls, aug)
    out = self._forward(torch.cat([x, x]), torch.cat([time_cond, time_cond]), both, None if aug is None else torch.cat([aug, aug]))
    c, u = out[:B], out[B:]
    phi = self._cfg_rescale
    if torch.is_grad_enabled():
      g = c + w * (c - u)
      if phi == 0.0:
        return g
      # the kernel's formula: the standard deviations and f in float64, f rounded to fp32 once
      std = lambda v: v.double().std(dim=(1, 2, 3), keepdim=True, unbiased=False)
      sd_c, sd_g = std(c), std(g)
      ok = torch.isfinite(sd_g) & (sd_g > 0)
      f = torch.where(ok, phi * (sd_c / torch.where(ok, sd_g, torch.ones_like(sd_g))) + (1.0 - phi), torch.ones_like(sd_g))
      return f.to(g.dtype) * g
    lib = self.engine().lib
    res = torch.empty_like(c)
    with _stk_lib.device_guard(c.device):
      if phi == 0.0:
        lib.cfg_combine_f32(c.data_ptr(), u.data_ptr(), w, res.data_ptr(), c.numel(), _stk_lib.stream_ptr(c.device))
      else:
        n = c.numel() // B
        ws = self._rescale_workspace(lib, B, n, c.device)
        lib.cfg_rescale_f32(c.data_ptr(), u.data_ptr(), w, phi, res.data_ptr(), B, n, ws.data_ptr(), ws.numel(),
                            _stk_lib.stream_ptr(c.device))
    return res

  def _rescale_workspace(self, lib, B, n, device):
    """The workspace of stk_cfg_rescale_f32 for B rows of n, allocated once per (B, n, device)."""
    ws = self._rescale_ws.get((B, n, device))
    if ws is None:
      if not getattr(lib, 'has_guided', False):
        raise NotImplementedError(f'{lib.path} ({lib.backend}) does not implement include/stk_guided.h: guidance rescale '
                                  f'needs stk_cfg_rescale_f32 (there is no other path)')
      ws = self._rescale_ws[(B, n, device)] = torch.empty(int(lib.guided_ws_bytes(B, n)), dtype=torch.uint8, device=device)
    return ws

  def _forward(self, x, time_cond, cls, aug=None):
    sigma = None
    if self.embedding_type == 'fourier':
      used_sigmas = time_cond
      if self.config.training.sde.lower() == 'reciprocal_sde':
        # dead branch in the reference too: the shipped configs say 'reciprocal_vesde' (ncsnpp.py:265)
        raise NotImplementedError
      emb_in = torch.log(used_sigmas)
    else:
      emb_in = time_cond
      if self.config.model.scale_by_sigma:
        used_sigmas = self.sigmas[time_cond.long()].to(torch.float32)
    if self.config.model.scale_by_sigma:
      sigma = used_sigmas
    return self.engine().apply(x, emb_in.to(torch.float32), sigma, cls, aug)

  # ------------------------------------------------------------------------------------------------
  # lowering: the walk of models/ncsnpp.py:258-432, emitted into the engine graph
  # ------------------------------------------------------------------------------------------------
  def _emit(self, g, B, H, W, need_xgrad):
    modules = self.all_modules
    cfg = self.config
    C = cfg.data.num_channels
    m_idx = 0
    g.act_code = self.act_code          # every gn_act(act=True) / silu() below applies the configured nonlinearity
    x = g.input('x', (B, C, H, W), needs_grad=need_xgrad)
    emb_in = g.input('emb', (B,))
    sigma = g.input('sigma', (B,)) if cfg.model.scale_by_sigma else None
    cls = g.input('cls', (B,)) if self.num_classes else None
    aug = g.input('aug', (B, self.augment_dim)) if self.augment_dim else None

    if self.embedding_type == 'fourier':
      temb = g.add(G.FourierEmbedding(g, emb_in, g.param(modules[m_idx].W)))
      m_idx += 1
    else:
      temb = g.add(G.TimestepEmbedding(g, emb_in, self.embed_dim))

    temb_proj, cols = None, {}
    if self.conditional:
      temb = g.linear(temb, modules[m_idx].weight, modules[m_idx].bias, name='temb.l0')
      m_idx += 1
      temb = g.linear(g.silu(temb, name='temb.act0'), modules[m_idx].weight, modules[m_idx].bias, name='temb.l1')
      m_idx += 1
      if cls is not None:
        temb = g.add(G.ClassEmbedding(g, temb, cls, g.param(self.class_emb.weight)))
      if aug is not None:
        temb = g.add(G.AugmentEmbedding(g, temb, aug, g.param(self.augment_emb.weight)))
      dense = self._dense_blocks()
      if dense:
        # all Dense_0(act(temb)) of the residual blocks as ONE GEMM over the stacked weights
        w0 = g.param(dense[0].Dense_0.weight)
        b0 = g.param(dense[0].Dense_0.bias)
        total = sum(b.Dense_0.weight.shape[0] for b in dense)
        tdim = dense[0].Dense_0.weight.shape[1]
        w_all = G.Tensor((total, tdim), 'param', w0.off, True, 'dense.W')
        w_all.goff = w0.off
        b_all = G.Tensor((total,), 'param', b0.off, True, 'dense.b')
        b_all.goff = b0.off
        col = 0
        for blk in dense:
          cols[id(blk)] = col
          col += blk.Dense_0.weight.shape[0]
        temb_proj = g.linear_t(g.silu(temb, name='temb.act1'), w_all, b_all, name='temb.proj')

    def res(mod, x1, x2=None, name='res'):
      return mod.emit(g, x1, x2, temb_proj, cols.get(id(mod), 0), name=name)

    if not cfg.data.centered:
      x = g.add(G.Affine(g, x, 2.0, -1.0, name='recentre'))   # x = 2x - 1

    input_pyramid = x if self.progressive_input != 'none' else None
    div = SQRT2 if self.skip_rescale else 1.0

    if self.fourier_feature:     # models/ncsnpp.py:305-308
      m_idx += 1
      hs = [layers.conv_emit(g, modules[m_idx], g.add(G.FixedFourier(g, x)), name='stem')]
    else:
      hs = [layers.conv_emit(g, modules[m_idx], x, name='stem')]
    m_idx += 1
    for i_level in range(self.num_resolutions):
      for i_block in range(self.num_res_blocks):
        h = res(modules[m_idx], hs[-1], name=f'd{i_level}.{i_block}')
        m_idx += 1
        if h.shape[-1] in self.attn_resolutions and self.attention:
          h = modules[m_idx].emit(g, h, name=f'd{i_level}.{i_block}.attn')
          m_idx += 1
        hs.append(h)

      if i_level != self.num_resolutions - 1:
        if self.resblock_type == 'ddpm':
          h = modules[m_idx].emit(g, hs[-1], name=f'd{i_level}.down')
          m_idx += 1
        elif self.auxiliary_resblock:
          h = res(modules[m_idx], hs[-1], name=f'd{i_level}.down')
          m_idx += 1

        if self.progressive_input == 'input_skip':
          input_pyramid = self.pyramid_downsample.emit(g, input_pyramid, name=f'd{i_level}.pyr')
          h = modules[m_idx].emit(g, input_pyramid, h, name=f'd{i_level}.combine')
          m_idx += 1
        elif self.progressive_input == 'residual':
          # input_pyramid = Downsample(input_pyramid); input_pyramid = (input_pyramid + h)/sqrt2; h = it
          input_pyramid = modules[m_idx].emit(g, input_pyramid, res=h, out_div=div, name=f'd{i_level}.pyr')
          m_idx += 1
          h = input_pyramid

        if self.auxiliary_resblock:
          hs.append(h)

    h = hs[-1]
    if not self.auxiliary_resblock:
      hs.pop()
    h = res(modules[m_idx], h, name='mid.0')
    m_idx += 1
    h = modules[m_idx].emit(g, h, name='mid.attn')
    m_idx += 1
    h = res(modules[m_idx], h, name='mid.1')
    m_idx += 1

    pyramid = None
    num_res_for_upsampling = self.num_res_blocks + 1 if self.auxiliary_resblock else self.num_res_blocks
    for i_level in reversed(range(self.num_resolutions)):
      for i_block in range(num_res_for_upsampling):
        h = res(modules[m_idx], h, hs.pop(), name=f'u{i_level}.{i_block}')   # cat([h, hs.pop()]) never materialised
        m_idx += 1

      if h.shape[-1] in self.attn_resolutions and self.attention:
        h = modules[m_idx].emit(g, h, name=f'u{i_level}.attn')
        m_idx += 1

      if self.progressive != 'none':
        if i_level == self.num_resolutions - 1:
          a = g.gn_act(h, None, modules[m_idx], act=True, name=f'u{i_level}.pyr.gn')
          m_idx += 1
          pyramid = layers.conv_emit(g, modules[m_idx], a, name=f'u{i_level}.pyr.conv')
          m_idx += 1
        else:
          if self.progressive == 'output_skip':
            pyramid = self.pyramid_upsample.emit(g, pyramid, name=f'u{i_level}.pyr.up')
            a = g.gn_act(h, None, modules[m_idx], act=True, name=f'u{i_level}.pyr.gn')
            m_idx += 1
            pyramid = layers.conv_emit(g, modules[m_idx], a, res=pyramid, name=f'u{i_level}.pyr.conv')
            m_idx += 1
          else:  # 'residual'
            pyramid = modules[m_idx].emit(g, pyramid, res=h, out_div=div, name=f'u{i_level}.pyr.up')
            m_idx += 1
            h = pyramid

      if i_level != 0:
        if self.resblock_type == 'ddpm':
          h = modules[m_idx].emit(g, h, name=f'u{i_level}.up')
          m_idx += 1
        elif self.auxiliary_resblock:
          h = res(modules[m_idx], h, name=f'u{i_level}.up')
          m_idx += 1

    assert not hs

    if self.progressive == 'output_skip':
      h = pyramid
    else:
      a = g.gn_act(h, None, modules[m_idx], act=True, name='head.gn')
      m_idx += 1
      h = layers.conv_emit(g, modules[m_idx], a, name='head.conv')
      m_idx += 1

    assert m_idx == len(modules)
    if cfg.model.scale_by_sigma:
      h = g.add(G.RowScale(g, h, sigma, name='by_sigma'))
    return h
