"""SimpleView: the reference's `MVModel` (openpoints/models/backbone/simpleview.py) over a fused depth rasteriser.

A cloud is drawn as six depth images (`PCViews.get_img`, openpoints/models/backbone/simpleview_util.py:235-292), a
ResNet-18 of BasicBlocks at `channels` width reads them and `MVFC` joins the six feature vectors.  The image layers are
PyTorch-ROCm's; the rasteriser is csrc/depth_views.hip:

  * `depth_views(points, rot, trans, H, W, size_x, size_y)`: points (B,N,3) under V views -> (B*V, H, W), image b*V + v
    = cloud b under view v.  One forward launch, one backward launch; no float atomic, no memset; the gradient flows
    through the depth only (the pixel coordinates pass through `ceil`), as it does in the reference.
  * `points2depth(points, H, W, size_x=4, size_y=4)`: the reference's function over camera-frame points.
  * `composed_points2depth` / `composed_depth_views`: the reference's composition in torch operations, for CPU tensors and
    `fused=False`.  What the kernel does not cover (CPU tensors, other dtypes and splat sizes, shapes outside its bounds)
    runs the composition and is counted by reason in COMPOSED_CALLS.

The transform is q = p R_v - t_v, summed left to right in fp32 in the kernel; the composition calls torch.matmul as the
reference does.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .fused import _call
from .pointnext import SmoothCrossEntropy

RESOLUTION = 128
TRANS = -1.4
SPLAT_SIZES = (1, 2, 4)
MAX_SPLATS = 16384         # apn_depth_views_max_splats(): N * size_x * size_y
MAX_PIXELS = 65536         # apn_depth_views_max_pixels(): H * W
MAX_VIEWS = 64             # apn_depth_views_max_views()
MAX_IMAGES = 2 ** 22 - 1   # apn_depth_views_max_images(): B * V workgroups of 1024 threads, below 2^32 threads in a grid
MAX_POINTS = 2 ** 31 - 1   # B * N: a thread per point in the backward

# calls that ran the composition instead of the kernel, by reason
COMPOSED_CALLS = {}


def euler2mat(angle):
    """Euler angles (3,) or (b,3) -> rotation matrices X(x) Y(y) Z(z), (3,3) or (b,3,3)."""
    if angle.dim() not in (1, 2):
        raise ValueError("euler2mat: angles must be (3,) or (b, 3)")
    x, y, z = angle.unbind(-1)
    zero = z.detach() * 0
    one = zero + 1
    view = list(angle.shape[:-1]) + [3, 3]

    def mat(*rows):
        return torch.stack(rows, dim=-1).reshape(view)
    cz, sz, cy, sy, cx, sx = torch.cos(z), torch.sin(z), torch.cos(y), torch.sin(y), torch.cos(x), torch.sin(x)
    zmat = mat(cz, -sz, zero, sz, cz, zero, zero, zero, one)
    ymat = mat(cy, zero, sy, zero, one, zero, -sy, zero, cy)
    xmat = mat(one, zero, zero, zero, cx, -sx, zero, sx, cx)
    return xmat @ ymat @ zmat


# ------------------------------------------------------------------ the reference's composition
def composed_points2depth(points, image_height, image_width, size_x=4, size_y=4, with_weight=False):
    """simpleview_util.py:60-171 restated: camera-frame points (B,N,3) -> (B,H,W); with_weight: also the per-pixel weight
    sum before its zeros are replaced by one.  About 45 launches, two scatter_add (float atomics on the GPU)."""
    for s in (size_x, size_y):
        if not (s == 1 or (s > 0 and s % 2 == 0)):
            raise ValueError("points2depth: a splat size is 1 or even")
    H, W = image_height, image_width
    B, N, _ = points.shape
    dev, dt = points.device, points.dtype
    eps = torch.full((1,), 1e-12, device=dev, dtype=dt)              # (a fill, not a host copy: capturable)
    z = points[:, :, 2]
    fx = (((points[:, :, 0] / (z + eps)) * (W / H) + 1) * H) / 2
    fy = (((points[:, :, 1] / (z + eps)) + 1) * W) / 2
    oi = torch.linspace(-size_x / 2, size_x / 2 - 1, size_x, device=dev, dtype=dt)
    oj = torch.linspace(-size_y / 2, size_y / 2 - 1, size_y, device=dev, dtype=dt)
    ex = (fx.unsqueeze(2) + oi).ceil().unsqueeze(3).expand(B, N, size_x, size_y)
    ey = (fy.unsqueeze(2) + oj).ceil().unsqueeze(2).expand(B, N, size_x, size_y)
    value = z.unsqueeze(2).unsqueeze(3).expand(B, N, size_x, size_y)
    mask = (ex >= 0) * (ex <= H - 1) * (ey >= 0) * (ey <= W - 1) * (value >= 0)
    weight = mask.to(dt) * (1 / (value + eps))
    weighted = value * weight
    # (the reference wraps the masked-out coordinates into the image and adds their zero weight there; they go to pixel 0
    # here, which adds the same zero and cannot index outside the image)
    coord = torch.where(mask, ex * W + ey, torch.zeros((), device=dev, dtype=dt)).reshape(B, -1).long()
    sw = torch.zeros(B, H * W, device=dev, dtype=dt).scatter_add(1, coord, weight.reshape(B, -1))
    sv = torch.zeros(B, H * W, device=dev, dtype=dt).scatter_add(1, coord, weighted.reshape(B, -1))
    img = (sv / (sw + (sw == 0).to(dt))).view(B, H, W)
    return (img, sw.view(B, H, W)) if with_weight else img


def composed_depth_views(points, rot, trans, image_height, image_width, size_x=1, size_y=1, with_weight=False):
    """`PCViews.get_img` restated: repeat_interleave, torch.matmul, the subtraction, then `composed_points2depth`."""
    B, V = points.shape[0], rot.shape[0]
    q = torch.matmul(torch.repeat_interleave(points, V, dim=0), rot.repeat(B, 1, 1)) - trans.reshape(V, 1, 3).repeat(B, 1, 1)
    return composed_points2depth(q, image_height, image_width, size_x, size_y, with_weight)


# ------------------------------------------------------------------ the kernel
def _check_views(rot, trans):
    """rot (V,3,3) and trans with 3 V elements, or neither: ValueError otherwise, whichever form then runs."""
    if rot is None and trans is None:
        return
    if rot is None or trans is None or not (torch.is_tensor(rot) and torch.is_tensor(trans)):
        raise ValueError("depth_views: rot and trans are both tensors, or both None")
    if rot.dim() != 3 or tuple(rot.shape[1:]) != (3, 3) or rot.shape[0] == 0:
        raise ValueError("depth_views: rot must be (V, 3, 3), got %s" % (tuple(rot.shape),))
    if trans.numel() != 3 * rot.shape[0] or trans.shape[-1] != 3:
        raise ValueError("depth_views: trans must be (V, 3) or (V, 1, 3) with rot's V = %d, got %s"
                         % (rot.shape[0], tuple(trans.shape)))


def _why_composed(points, rot, trans, H, W, size_x, size_y):
    """None if the kernel takes the call, else the reason it does not.  Every tensor whose pointer the kernel would be
    handed is checked here: device, dtype and (`_check_views`) shape."""
    _check_views(rot, trans)
    if rot is not None and not (rot.device == points.device and trans.device == points.device):
        return "rot / trans on another device than the points"          # (the composition then raises torch's own error)
    if not points.is_cuda:
        return "cpu tensor"
    if points.dtype != torch.float32:
        return "dtype %s" % points.dtype
    if rot is not None and not (rot.dtype == torch.float32 and trans.dtype == torch.float32):
        return "rot %s / trans %s" % (rot.dtype, trans.dtype)
    if points.dim() != 3 or points.shape[-1] != 3:
        return "%d-d input" % points.dim()
    if size_x not in SPLAT_SIZES or size_y not in SPLAT_SIZES:
        return "splat %dx%d" % (size_x, size_y)
    B, N, _ = points.shape
    V = 1 if rot is None else rot.shape[0]
    if not (0 < H * W <= MAX_PIXELS and 0 < N * size_x * size_y <= MAX_SPLATS and 0 < V <= MAX_VIEWS):
        return "shape outside the kernel's bounds (H*W %d, N*sx*sy %d, V %d)" % (H * W, N * size_x * size_y, V)
    if not (0 < B * V <= MAX_IMAGES and B * N <= MAX_POINTS):
        return "batch %d outside the grid bounds" % B
    return None


def supported(points, rot, trans, H, W, size_x=1, size_y=1):
    return _why_composed(points, rot, trans, H, W, size_x, size_y) is None


class _DepthViews(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, rot, trans, H, W, size_x, size_y):
        points = points.contiguous()
        B, N, _ = points.shape
        dev = points.device
        V = 1
        if rot is not None:
            rot, trans = rot.contiguous(), trans.reshape(-1, 3).contiguous()
            V = rot.shape[0]
        img = torch.empty(B * V, H, W, dtype=torch.float32, device=dev)
        sw = torch.empty(B * V, H, W, dtype=torch.float32, device=dev)
        _call("apn_depth_views_fwd", dev, B, N, V, H, W, size_x, size_y, points.data_ptr(),
              rot.data_ptr() if rot is not None else None, trans.data_ptr() if rot is not None else None,
              img.data_ptr(), sw.data_ptr())
        ctx.save_for_backward(points, rot, trans, img, sw)
        ctx.geom = (V, H, W, size_x, size_y)
        ctx.mark_non_differentiable(sw)
        return img, sw

    @staticmethod
    def backward(ctx, g, _g_sw):
        points, rot, trans, img, sw = ctx.saved_tensors
        V, H, W, size_x, size_y = ctx.geom
        B, N, _ = points.shape
        g = g.contiguous().float()
        dpoints = torch.empty_like(points)
        _call("apn_depth_views_bwd", points.device, B, N, V, H, W, size_x, size_y, points.data_ptr(),
              rot.data_ptr() if rot is not None else None, trans.data_ptr() if rot is not None else None,
              g.data_ptr(), img.data_ptr(), sw.data_ptr(), dpoints.data_ptr())
        return dpoints, None, None, None, None, None, None


def _rasterise(points, rot, trans, H, W, size_x, size_y, fused, with_weight):
    H, W, size_x, size_y = int(H), int(W), int(size_x), int(size_y)
    if fused is not False:
        why = _why_composed(points, rot, trans, H, W, size_x, size_y)
        if why is None:
            _lib.load()
            img, sw = _DepthViews.apply(points, rot, trans, H, W, size_x, size_y)
            return (img, sw) if with_weight else img
        COMPOSED_CALLS[why] = COMPOSED_CALLS.get(why, 0) + 1
    else:
        _check_views(rot, trans)
    if rot is None:
        return composed_points2depth(points, H, W, size_x, size_y, with_weight)
    return composed_depth_views(points, rot, trans, H, W, size_x, size_y, with_weight)


def points2depth(points, image_height, image_width, size_x=4, size_y=4, fused=None, with_weight=False):
    """simpleview_util.py:136-171: camera-frame points (B,N,3) -> depth images (B, image_height, image_width)."""
    return _rasterise(points, None, None, image_height, image_width, size_x, size_y, fused, with_weight)


def depth_views(points, rot, trans, image_height, image_width, size_x=1, size_y=1, fused=None, with_weight=False):
    """points (B,N,3), rot (V,3,3), trans (V,3) or (V,1,3) -> (B*V, H, W): cloud b under view v is image b*V + v."""
    return _rasterise(points, rot, trans, image_height, image_width, size_x, size_y, fused, with_weight)


class PCViews:
    """simpleview_util.py:235-292: the six (euler angles, translation) views; the matrices are built once in float32 and
    kept per device the first time a cloud of that device arrives (no copy afterwards: a captured step holds none)."""

    VIEWS = (((0 * np.pi / 2, 0, np.pi / 2), (0, 0, TRANS)),
             ((1 * np.pi / 2, 0, np.pi / 2), (0, 0, TRANS)),
             ((2 * np.pi / 2, 0, np.pi / 2), (0, 0, TRANS)),
             ((3 * np.pi / 2, 0, np.pi / 2), (0, 0, TRANS)),
             ((0, -np.pi / 2, np.pi / 2), (0, 0, TRANS)),
             ((0, np.pi / 2, np.pi / 2), (0, 0, TRANS)))

    def __init__(self, resolution=RESOLUTION, fused=None):
        views = np.asarray(self.VIEWS)
        self.num_views = len(self.VIEWS)
        self.resolution, self.fused = resolution, fused
        self.rot_mat = euler2mat(torch.tensor(views[:, 0, :]).float()).transpose(1, 2).contiguous()
        self.translation = torch.tensor(views[:, 1, :]).float().unsqueeze(1)
        self._on = {}

    def matrices(self, device):
        """(rot (6,3,3), translation (6,1,3)) on `device`."""
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = (self.rot_mat.to(device), self.translation.to(device))
        return self._on[device]

    def get_img(self, points):
        """points (B,N,3) -> (B * num_views, resolution, resolution)."""
        rot, trans = self.matrices(points.device)
        if points.dtype != rot.dtype:
            rot, trans = rot.to(points.dtype), trans.to(points.dtype)
        return depth_views(points, rot, trans, self.resolution, self.resolution, 1, 1, fused=self.fused)

    @staticmethod
    def point_transform(points, rot_mat, translation):
        """points (b,n,3), rot_mat (b,3,3), translation (b,1,3) -> points rot_mat - translation."""
        return torch.matmul(points, rot_mat.to(points.device)) - translation.to(points.device)


# ------------------------------------------------------------------ the model
class Squeeze(nn.Module):
    def forward(self, inp):
        return inp.squeeze()


class BatchNormPoint(nn.Module):
    def __init__(self, feat_size):
        super().__init__()
        self.feat_size = feat_size
        self.bn = nn.BatchNorm1d(feat_size)

    def forward(self, x):
        if x.dim() != 3 or x.shape[2] != self.feat_size:
            raise ValueError("BatchNormPoint: input must be (b, n, %d)" % self.feat_size)
        s1, s2, s3 = x.shape
        return self.bn(x.reshape(s1 * s2, s3)).view(s1, s2, s3)


class MVFC(nn.Module):
    """simpleview.py:33-58: the head over the `num_views` feature vectors of a cloud."""

    def __init__(self, num_views, in_features, out_features, dropout):
        super().__init__()
        self.num_views, self.in_features = num_views, in_features
        self.model = nn.Sequential(
            BatchNormPoint(in_features),
            nn.Dropout(dropout),            # before the concatenation: each view drops its own features
            nn.Flatten(),
            nn.Linear(in_features * num_views, in_features),
            nn.BatchNorm1d(in_features),
            nn.ReLU(),
            nn.Dropout(dropout),
            nn.Linear(in_features, out_features, bias=True))

    def forward(self, feat):
        return self.model(feat.view(-1, self.num_views, self.in_features))


class BasicBlock(nn.Module):
    """openpoints/models/backbone/resnet.py:35-72."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x)))))
        out = out + (x if self.downsample is None else self.downsample(x))
        return self.relu(out)


def resnet18_layers(channels):
    """layer1..layer4 of the reference's ResNet(BasicBlock, [2,2,2,2], feature_size=channels, zero_init_residual=True)
    and its average pool: widths channels, 2x, 4x, 8x; kaiming-normal (fan_out) convolutions, the second BatchNorm of
    every block starting at zero.  -> (modules, channels * 8)"""
    layers, inplanes = [], channels
    for k, stride in enumerate((1, 2, 2, 2)):
        planes = channels << k
        down = None
        if stride != 1 or inplanes != planes:
            down = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride=stride, bias=False), nn.BatchNorm2d(planes))
        layers.append(nn.Sequential(BasicBlock(inplanes, planes, stride, down), BasicBlock(planes, planes)))
        inplanes = planes
    for layer in layers:
        for m in layer.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
        for m in layer.modules():
            if isinstance(m, BasicBlock):
                nn.init.constant_(m.bn2.weight, 0)
    return layers + [nn.AdaptiveAvgPool2d((1, 1))], inplanes


class MVModel(nn.Module):
    """simpleview.py:61-153.  `resolution` is honoured here (the reference reads a module constant, 128: the default).
    fused: None / True: the rasteriser kernel wherever it applies; False: the composition."""

    def __init__(self, task='cls', backbone='resnet18', channels=16, num_classes=15, resolution=128,
                 use_img_transform=False, fused=None, dropout=0.5, **kwargs):
        super().__init__()
        if task != 'cls':
            raise NotImplementedError("MVModel: task %r" % (task,))
        if use_img_transform:
            raise NotImplementedError("MVModel: use_img_transform (the reference's Zoom image transform) is not built")
        self.task, self.num_classes, self.dropout, self.channels = task, num_classes, dropout, channels
        self.resolution = resolution
        self.pc_views = PCViews(resolution=resolution, fused=fused)
        self.num_views = self.pc_views.num_views
        img_layers, in_features = self.get_img_layers(backbone, channels=channels)
        self.img_model = nn.Sequential(*img_layers)
        self.final_fc = MVFC(num_views=self.num_views, in_features=in_features, out_features=num_classes, dropout=dropout)
        self.img_transform = None

    def set_fused(self, fused):
        self.pc_views.fused = fused
        return self

    def forward(self, pc):
        if hasattr(pc, 'keys'):
            pc = pc['pos']
        return self.final_fc(self.img_model(self.get_img(pc)))

    def forward_cls_feat(self, pc):
        return self.forward(pc)

    def get_img(self, pc):
        """(B,N,3) -> (B * num_views, 1, resolution, resolution)"""
        return self.pc_views.get_img(pc).unsqueeze(3).permute(0, 3, 1, 2)

    @staticmethod
    def get_img_layers(backbone, channels):
        if backbone != 'resnet18':
            raise NotImplementedError("MVModel: backbone %r (BasicBlock ResNet-18 only)" % (backbone,))
        main_layers, in_features = resnet18_layers(channels)
        return [nn.Conv2d(1, channels, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), bias=False),
                nn.BatchNorm2d(channels, eps=1e-05, momentum=0.1, affine=True, track_running_stats=True),
                nn.ReLU(inplace=True),
                *main_layers,
                Squeeze()], in_features


class SimpleViewClassifier(nn.Module):
    """`MVModel` behind the classifiers' interface (`PointMlpClassifier`'s shape): `encoder` is the whole reference model,
    head included; SmoothCrossEntropy(0.3).  Only data['pos'] is read."""

    def __init__(self, num_classes=15, fused=None, **model_args):
        super().__init__()
        self.encoder = MVModel(num_classes=num_classes, fused=fused, **model_args)
        self.criterion = SmoothCrossEntropy(0.3)

    def forward(self, data):
        return self.encoder(data)

    def get_logits_loss(self, data, gt):
        logits = self.forward(data)
        return logits, self.criterion(logits, gt.long())
