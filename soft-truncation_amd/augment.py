"""Non-leaky augmentation (Karras et al. 2022, "Elucidating the Design Space of Diffusion-Based Generative Models", appendix
F.2): every training image is flipped, scaled, rotated, stretched and shifted at random, and the network is TOLD what was
done -- nine augmentation labels enter its time embedding (config.model.augment_dim, engine.graph.AugmentEmbedding) -- so it
learns the augmented distribution conditionally and samples, with the labels at zero, from the clean one.

`AugmentPipe` draws the per-sample transforms on the HOST, from a CPU generator of its own (the device RNG stream of the
losses is untouched), builds each sample's inverse map in float64, and applies all of it in ONE launch of stk_aug_warp_f32
(include/stk_augment.h: flip, 2x FIR upsampling of the reflect-extended plane, bilinear warp, 2x FIR downsampling; samples
without a geometric part are copied bit for bit).  The [B, 8] parameter rows and [B, 9] labels go up from pinned memory
without blocking; nothing is read back and nothing synchronises.

Each of the six transforms fires with probability p, independently; its draw is 0 otherwise.
  transform       draw                          forward map on the image                          labels
  x-flip, y-flip  w in {0, 1} each              flip                                              w                 (2)
  scale           w ~ N(0, 1)                   scale by 2^(0.2 w)                                w                 (1)
  rotation        w ~ U(-pi, pi)                rotate by w                                       cos w - 1, sin w  (2)
  anisotropy      phi ~ U(-pi, pi), r ~ N(0,1)  R(phi) diag(2^(0.2 r), 2^(-0.2 r)) R(-phi)        r cos phi, r sin phi (2)
  translation     w ~ N(0, 1)^2                 shift by 0.125 (W w0, H w1) pixels                w0, w1            (2)
composed in that order (scale first, translation last).

Differences from EDM's pipe, all deliberate: the low-pass is a SYMMETRIC 12-tap Kaiser-windowed half-band sinc (EDM's sym6
wavelet taps are not symmetric; the kernel's periodic lattice needs f[k] = f[T-1-k], and another symmetric filter can be
given); the boundary is the reflection of the plane itself, so no margin is computed from the batch's matrices (EDM's margin
costs a max() read-back per batch); integer-pixel translations, 90-degree rotations as a separate transform, and the colour
and noise augmentations are absent; planes are at most 64 x 64.
"""
import ctypes

import numpy as np
import torch

from .engine import lib as stk_lib
from .op import _backend

NUM_LABELS = 9
TRANSFORMS = ('xflip', 'yflip', 'scale', 'rotate', 'aniso', 'translate')


def default_filter():
  """The 12 taps of the default low-pass: sinc((k - 5.5) / 2) kaiser(12, 8)[k], normalised to sum 1 in float64, as fp32."""
  k = np.arange(12, dtype=np.float64)
  f = np.sinc((k - 5.5) / 2.0) * np.kaiser(12, 8.0)
  return (f / f.sum()).astype(np.float32)


def check_probability(p, key='config.training.augment'):
  try:
    p = float(p)
  except (TypeError, ValueError):
    raise ValueError(f'{key} must be a probability in [0, 1], got {p!r}') from None
  if not 0.0 <= p <= 1.0:
    raise ValueError(f'{key} must be a probability in [0, 1], got {p!r}')
  return p


def check_filter(taps, key='config.training.augment_filter'):
  """`taps` as the fp32 array the kernel takes.  ValueError: not 1-D, an odd or zero count, more than 12, a tap that is not
  finite, f[k] != f[T-1-k] (in fp32: what the kernel compares)."""
  f = np.asarray(default_filter() if taps is None else taps, dtype=np.float32)
  if f.ndim != 1 or f.size == 0 or f.size % 2 or f.size > 12 or not np.isfinite(f).all():
    raise ValueError(f'{key} must be an even number (at most 12) of finite taps, got shape {f.shape}')
  if not np.array_equal(f, f[::-1]):
    raise ValueError(f'{key} must be symmetric, f[k] = f[T-1-k] (stk_aug_warp_f32 returns STK_EUNSUPPORTED otherwise): the '
                     f'upsampled plane is indexed through its mirror symmetry, which an unsymmetric filter such as a sym6 '
                     f'wavelet low-pass does not have')
  return np.ascontiguousarray(f)


def shape_ok(H, W, T):
  """The rule of stk_aug_ok, for checks made before a library is bound."""
  return 8 <= H <= 64 and 8 <= W <= 64 and H % 2 == 0 and W % 2 == 0 and 2 <= T <= 12 and T % 2 == 0


def _rotation(a):
  c, s = np.cos(a), np.sin(a)
  return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)


class AugmentPipe:
  """``pipe(images) -> (augmented, labels)`` on the device; ``pipe.draw(B, H, W) -> (params, labels)`` on the host.

  p: the probability of each transform;  filter: symmetric low-pass taps (None: `default_filter`);  seed: of the pipe's own
  CPU generator."""

  def __init__(self, p, filter=None, seed=0):
    self.p = check_probability(p, 'AugmentPipe: p')
    self.filter = check_filter(filter, 'AugmentPipe: filter')
    self._taps = (ctypes.c_float * len(self.filter))(*self.filter.tolist())     # the HOST pointer the entry reads
    self.generator = torch.Generator(device='cpu')
    self.generator.manual_seed(int(seed))

  def sample(self, B):
    """The raw draws of B samples, float64 numpy, zeros where a transform does not fire: dict with 'fires' [B, 6] bool (in the
    order of TRANSFORMS), 'xflip', 'yflip', 'scale', 'rotate', 'aniso_phi', 'aniso_r' [B] and 'translate' [B, 2]."""
    g = self.generator
    fires = (torch.rand(B, 6, generator=g, dtype=torch.float64) < self.p).numpy()
    flips = torch.randint(0, 2, (B, 2), generator=g).to(torch.float64).numpy()
    normal = torch.randn(B, 4, generator=g, dtype=torch.float64).numpy()
    angle = ((torch.rand(B, 2, generator=g, dtype=torch.float64) * 2 - 1) * np.pi).numpy()
    on = fires.astype(np.float64)
    return {
      'fires': fires,
      'xflip': flips[:, 0] * on[:, 0], 'yflip': flips[:, 1] * on[:, 1],
      'scale': normal[:, 0] * on[:, 2],
      'rotate': angle[:, 0] * on[:, 3],
      'aniso_phi': angle[:, 1] * on[:, 4], 'aniso_r': normal[:, 1] * on[:, 4],
      'translate': normal[:, 2:4] * on[:, 5:6],
    }

  @staticmethod
  def forward_maps(raw, H, W):
    """[B, 3, 3] float64: the forward map of every sample on centred pixel coordinates (x, y, 1), flips excluded --
    translation o anisotropy o rotation o scale."""
    B = raw['scale'].shape[0]
    s = 2.0 ** (0.2 * raw['scale'])
    lin = s[:, None, None] * np.broadcast_to(np.eye(2), (B, 2, 2))
    lin = _rotation(raw['rotate']) @ lin
    r = 2.0 ** (0.2 * raw['aniso_r'])
    stretch = np.zeros((B, 2, 2))
    stretch[:, 0, 0], stretch[:, 1, 1] = r, 1.0 / r
    lin = _rotation(raw['aniso_phi']) @ stretch @ _rotation(-raw['aniso_phi']) @ lin
    G = np.zeros((B, 3, 3))
    G[:, :2, :2] = lin
    G[:, 0, 2] = 0.125 * W * raw['translate'][:, 0]
    G[:, 1, 2] = 0.125 * H * raw['translate'][:, 1]
    G[:, 2, 2] = 1.0
    return G

  @staticmethod
  def inverse_maps(G):
    """[B, 3, 3] float64: the inverses of `forward_maps`, closed form (the maps are affine with determinant s^2 > 0)."""
    lin, tau = G[:, :2, :2], G[:, :2, 2]
    det = lin[:, 0, 0] * lin[:, 1, 1] - lin[:, 0, 1] * lin[:, 1, 0]
    A = np.empty_like(lin)
    A[:, 0, 0], A[:, 0, 1] = lin[:, 1, 1] / det, -lin[:, 0, 1] / det
    A[:, 1, 0], A[:, 1, 1] = -lin[:, 1, 0] / det, lin[:, 0, 0] / det
    inv = np.zeros_like(G)
    inv[:, :2, :2] = A
    inv[:, :2, 2] = -np.einsum('bij,bj->bi', A, tau)
    inv[:, 2, 2] = 1.0
    return inv

  @staticmethod
  def labels_of(raw):
    """[B, 9] float64, the columns of the table in the module docstring."""
    w, phi, r = raw['rotate'], raw['aniso_phi'], raw['aniso_r']
    return np.stack([raw['xflip'], raw['yflip'], raw['scale'], np.cos(w) - 1.0, np.sin(w), r * np.cos(phi), r * np.sin(phi),
                     raw['translate'][:, 0], raw['translate'][:, 1]], axis=1)

  def params_of(self, raw, H, W):
    """[B, 8] fp32 rows (fx, fy, a00, a01, a10, a11, t0, t1) of include/stk_augment.h: float64 throughout, rounded once.  A
    sample whose four geometric transforms all draw 0 gets the identity row exactly (2^0 = 1, cos 0 = 1, sin 0 = 0)."""
    inv = self.inverse_maps(self.forward_maps(raw, H, W))
    rows = np.concatenate([raw['xflip'][:, None], raw['yflip'][:, None], inv[:, :2, :2].reshape(-1, 4), inv[:, :2, 2]], axis=1)
    return rows.astype(np.float32)

  def draw(self, B, H, W):
    """(params [B, 8], labels [B, 9]), fp32 torch tensors on the host."""
    raw = self.sample(B)
    return torch.from_numpy(self.params_of(raw, H, W)), torch.from_numpy(self.labels_of(raw).astype(np.float32))

  def check_shape(self, H, W, key='config.data.image_size'):
    if not shape_ok(H, W, len(self.filter)):
      raise ValueError(f'{key}: the augmentation takes planes with even sides in [8, 64] (stk_aug_ok), got {H} x {W}; larger '
                       f'planes are refused, not emulated')

  def __call__(self, images):
    """images [B, C, H, W] fp32 on the device -> (augmented [B, C, H, W], labels [B, 9]) on the device, on the current stream."""
    if images.dim() != 4 or images.dtype != torch.float32:
      raise ValueError(f'AugmentPipe takes [B, C, H, W] float32 images, got {tuple(images.shape)} {images.dtype}')
    lib = _backend.get()
    if not getattr(lib, 'has_augment', False):
      raise NotImplementedError(f'{lib.path} ({lib.backend}) does not implement include/stk_augment.h: the augmentation '
                                f'needs stk_aug_warp_f32 (there is no other path)')
    _backend.check(images, lib)
    B, C, H, W = images.shape
    self.check_shape(H, W, 'AugmentPipe')
    images = images.contiguous()
    params, labels = self.draw(B, H, W)
    both = torch.cat([params.reshape(-1), labels.reshape(-1)])        # one upload: the 8 B parameters, then the 9 B labels
    if images.is_cuda:
      # a fresh pinned block per batch: torch's host allocator takes it back only once the copy below has run
      both = both.pin_memory().to(images.device, non_blocking=True)
    params, labels = both[:8 * B].view(B, 8), both[8 * B:].view(B, NUM_LABELS)
    out = torch.empty_like(images)
    with stk_lib.device_guard(images.device):
      lib.aug_warp_f32(images.data_ptr(), params.data_ptr(), ctypes.cast(self._taps, ctypes.c_void_p), len(self.filter),
                       out.data_ptr(), B, C, H, W, stk_lib.stream_ptr(images.device))
    return out, labels
