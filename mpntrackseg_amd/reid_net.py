"""Host-side mirror of the reference's ReID CNN (``/root/reference/src/mot_neural_solver/models/resnet.py``: the torchreid
ResNet50 with two fully connected layers, ``resnet50_fc256``): the same attribute names and ``Sequential`` indices, so the
reference's ``state_dict`` keys load (``layerL.B.downsample.{0,1}.*``, ``fc.{0,1,3,4}.*``, ``classifier.*``, the BatchNorm
buffers).  There is no ``pretrained`` argument and no URL table: this module never fetches anything; weights come from a file
through ``load_pretrained_weights``.

``ResNet.forward`` runs the stock PyTorch-ROCm (MIOpen) modules and returns ``(f, v)`` as the reference does (``resnet.py:271-279``):
the ``[n, 2048, H / 16, W / 16]`` feature map -- the tracker's node-core input -- and the ``[n, 256]`` ReID vector.  It is the
comparator and the default.

``ResNet.forward_native`` is the opt-in no-grad inference forward through the C ABI (csrc/conv_strided.hip): the stem as one
``mpnhip_conv2d_affine_forward`` (conv1 + bn1 + ReLU) and one ``mpnhip_maxpool2d_forward``, every bottleneck as three such
convolutions (four with its downsample; the last carries the residual add and the ReLU), ``mpnhip_avgpool`` over the pixels and
one ``mpnhip_linear`` per ``Linear + BatchNorm1d + ReLU`` of ``fc`` with the BatchNorm folded into weight and bias.  No MIOpen
algorithm search, and the bits of both results do not depend on the batch: an image's ``f`` and ``v`` are the same alone and inside
any batch.  For ``f`` that is the convolution kernel's contract.  For ``v`` it rests on two facts of the existing operators:
``mpnhip_avgpool`` sums a row by its length alone, and ``mpnhip_linear`` (``launch_gemm``, csrc/gemm.hip) runs one kernel with one
chain per output for every row count below 8192 at these widths -- so a slice never holds more than ``MAX_SLICE`` = 8191 crops.

The folded constants ``scale = gamma / sqrt(var + eps)``, ``shift = beta - mean * scale`` and the folded ``fc`` weights are
computed in float64 and rounded once to the parameters' dtype (float32 for every module ``forward_native`` accepts); they are
cached on the module by ``prepare_native()`` and dropped by ``load_state_dict``, ``.to()`` (anything that goes through
``_apply``) and ``.train()`` / ``.eval()``."""
import ctypes as C
from collections import OrderedDict

import torch
from torch import nn

from . import capi
from .capi import MpnhipError
from .cnn import _image_dense, _out_tensor


MAX_SLICE = 8191      # crops per slice of forward_native: launch_gemm changes its kernel (hence v's summation) at 8192 rows


# ------------------------------------------------------------------------------------------------ operators
def _conv_out(size, stride):
    return (int(size) - 1) // int(stride) + 1


def _dense_input(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise MpnhipError("%s must be a float32 [N, C, H, W] device tensor" % what)
    capi.require_device(x)
    return x if _image_dense(x) else capi.f32c(x)


def _vec(t, n, like, what):
    if t is None:
        return None
    t = capi.f32c(t.detach())
    capi.require_device(t)
    if t.numel() != n or t.device != like.device:
        raise MpnhipError("%s must hold %d floats on %s" % (what, n, like.device))
    return t


def conv2d_affine_native(x, weight, scale, shift, stride=1, residual=None, relu=False, out=None):
    """``mpnhip_conv2d_affine_forward``: Conv2d(k = 1 | 3 | 7, stride 1 | 2, padding k // 2, no bias) on ``x`` [N, cin, H, W]
    with ``weight`` [cout, cin, k, k], then ``* scale + shift`` per output channel (either may be None), ``+ residual``
    ([N, cout, Hout, Wout] or None) and the ReLU.  ``out`` (optional) may be a channel slice of a wider tensor; it must not
    overlap ``x`` or ``residual``.  No autograd."""
    xx = _dense_input(x, "x")
    w = capi.f32c(weight.detach())
    capi.require_device(w)
    n, cin, h, wd = xx.shape
    if w.dim() != 4 or int(w.shape[1]) != cin or w.shape[2] != w.shape[3] or w.device != xx.device:
        raise MpnhipError("weight %s does not fit %d input channels on %s" % (tuple(w.shape), cin, xx.device))
    cout, k = int(w.shape[0]), int(w.shape[2])
    ho, wo = _conv_out(h, stride), _conv_out(wd, stride)
    sc, sh = _vec(scale, cout, xx, "scale"), _vec(shift, cout, xx, "shift")
    res = None
    if residual is not None:
        res = _dense_input(residual, "residual")
        if tuple(res.shape) != (n, cout, ho, wo) or res.device != xx.device:
            raise MpnhipError("residual must be [%d, %d, %d, %d] on %s" % (n, cout, ho, wo, xx.device))
    y = _out_tensor(out, (n, cout, ho, wo), xx)
    a = capi.ConvAffineArgs()
    a.x, a.x_stride, a.weight = xx.data_ptr(), xx.stride(0), w.data_ptr()
    a.scale, a.shift = (sc.data_ptr() if sc is not None else None), (sh.data_ptr() if sh is not None else None)
    a.residual, a.residual_stride = (res.data_ptr(), res.stride(0)) if res is not None else (None, 0)
    a.relu, a.out, a.out_stride, a.n_images = int(bool(relu)), y.data_ptr(), y.stride(0), int(n)
    a.cin, a.cout, a.H, a.W, a.ksize, a.stride = int(cin), cout, int(h), int(wd), k, int(stride)
    with torch.cuda.device(y.device):
        capi.check(capi.load().mpnhip_conv2d_affine_forward(C.byref(a), capi.stream_ptr()), "mpnhip_conv2d_affine_forward")
    return y


def maxpool2d_native(x, out=None):
    """``mpnhip_maxpool2d_forward``: MaxPool2d(3, stride 2, padding 1) on ``x`` [N, C, H, W].  No autograd."""
    xx = _dense_input(x, "x")
    n, c, h, wd = xx.shape
    y = _out_tensor(out, (n, c, _conv_out(h, 2), _conv_out(wd, 2)), xx)
    with torch.cuda.device(y.device):
        capi.check(capi.load().mpnhip_maxpool2d_forward(capi.ptr(xx), xx.stride(0), int(n), int(c), int(h), int(wd), capi.ptr(y),
                                                        y.stride(0), capi.stream_ptr()), "mpnhip_maxpool2d_forward")
    return y


def fold_batchnorm(bn):
    """``(scale, shift)`` of an eval-mode BatchNorm, ``gamma / sqrt(var + eps)`` and ``beta - mean * scale``: float64 arithmetic,
    one rounding to the module's dtype."""
    var, mean = bn.running_var.detach().double(), bn.running_mean.detach().double()
    gamma = bn.weight.detach().double() if bn.weight is not None else torch.ones_like(var)
    beta = bn.bias.detach().double() if bn.bias is not None else torch.zeros_like(var)
    scale = gamma / torch.sqrt(var + bn.eps)
    shift = beta - mean * scale
    dtype = bn.running_var.dtype
    return scale.to(dtype).contiguous(), shift.to(dtype).contiguous()


def fold_linear_batchnorm(linear, bn):
    """``(weight, bias)`` of ``bn(linear(x))`` as one Linear, float64 arithmetic, one rounding to the module's dtype."""
    var, mean = bn.running_var.detach().double(), bn.running_mean.detach().double()
    gamma = bn.weight.detach().double() if bn.weight is not None else torch.ones_like(var)
    beta = bn.bias.detach().double() if bn.bias is not None else torch.zeros_like(var)
    scale = gamma / torch.sqrt(var + bn.eps)
    w = linear.weight.detach().double() * scale[:, None]
    b0 = linear.bias.detach().double() if linear.bias is not None else torch.zeros_like(var)
    b = (b0 - mean) * scale + beta
    dtype = linear.weight.dtype
    return w.to(dtype).contiguous(), b.to(dtype).contiguous()


# ------------------------------------------------------------------------------------------------ modules
class Bottleneck(nn.Module):
    """1 x 1 -> 3 x 3 (carries the stride) -> 1 x 1 (x 4 channels), each with its BatchNorm, around a shortcut."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        out = out + (x if self.downsample is None else self.downsample(x))
        return self.relu(out)


class ResNet(nn.Module):
    """``models/resnet.py``'s ResNet for the block types this project runs (``Bottleneck``), see the module docstring."""

    def __init__(self, num_classes, loss, block, layers, last_stride=2, fc_dims=None, dropout_p=None):
        super().__init__()
        self.loss = loss
        self.block = block
        self.dropout_p = dropout_p
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0], 1)
        self.layer2 = self._make_layer(block, 128, layers[1], 2)
        self.layer3 = self._make_layer(block, 256, layers[2], 2)
        self.layer4 = self._make_layer(block, 512, layers[3], last_stride)
        self.global_avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.feature_dim = 512 * block.expansion
        self.fc = self._construct_fc_layer(fc_dims, 512 * block.expansion, dropout_p)
        self.classifier = nn.Linear(self.feature_dim, num_classes)
        self._native = None
        self._init_params()

    def _make_layer(self, block, planes, blocks, stride):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, 1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
        stack = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        stack += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*stack)

    def _construct_fc_layer(self, fc_dims, input_dim, dropout_p=None):
        if fc_dims is None:
            self.feature_dim = input_dim
            return None
        assert isinstance(fc_dims, (list, tuple)), 'fc_dims must be either a list or a tuple, but got %s' % type(fc_dims)
        stack = []
        for dim in fc_dims:
            stack += [nn.Linear(input_dim, dim), nn.BatchNorm1d(dim), nn.ReLU(inplace=True)]
            if dropout_p is not None:
                stack.append(nn.Dropout(p=dropout_p))
            input_dim = dim
        self.feature_dim = fc_dims[-1]
        return nn.Sequential(*stack)

    def _init_params(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.constant_(m.bias, 0)

    # ---- the stock forward (resnet.py:260-279)
    def featuremaps(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))

    def forward(self, x):
        f = self.featuremaps(x)
        v = self.global_avgpool(f)
        v = v.view(v.size(0), -1)
        return (f, self.fc(v)) if self.fc is not None else (f, v)

    # ---- whatever changes the parameters or the mode drops the folded constants
    def load_state_dict(self, *args, **kw):
        self._native = None
        return super().load_state_dict(*args, **kw)

    def _apply(self, *args, **kw):
        self._native = None
        return super()._apply(*args, **kw)

    def train(self, mode=True):
        self._native = None
        return super().train(mode)

    # ---- the native forward
    def conv_layers(self, H, W):
        """Every convolution of ``featuremaps`` in execution order for an ``H x W`` input, as dicts: ``name`` (the Conv2d's name
        in the module tree), ``bn`` (its BatchNorm's), ``cin, cout, k, stride, H, W`` (input size), ``Hout, Wout``."""
        out = []

        def add(name, bn, conv, h, w):
            s = int(conv.stride[0])
            out.append(dict(name=name, bn=bn, cin=conv.in_channels, cout=conv.out_channels, k=int(conv.kernel_size[0]), stride=s, H=h, W=w,
                            Hout=_conv_out(h, s), Wout=_conv_out(w, s)))
            return out[-1]["Hout"], out[-1]["Wout"]

        h, w = add("conv1", "bn1", self.conv1, H, W)
        h, w = _conv_out(h, 2), _conv_out(w, 2)
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(self, "layer%d" % li)):
                p = "layer%d.%d." % (li, bi)
                add(p + "conv1", p + "bn1", blk.conv1, h, w)
                h2, w2 = add(p + "conv2", p + "bn2", blk.conv2, h, w)
                if blk.downsample is not None:
                    add(p + "downsample.0", p + "downsample.1", blk.downsample[0], h, w)
                add(p + "conv3", p + "bn3", blk.conv3, h2, w2)
                h, w = h2, w2
        return out

    def output_shapes(self, H, W):
        """``((C, h, w) of an image of f, width of v)`` for an ``H x W`` input"""
        last = self.conv_layers(H, W)[-1]
        return (last["cout"], last["Hout"], last["Wout"]), self.feature_dim

    def _fc_triples(self):
        mods = list(self.fc) if self.fc is not None else []
        if len(mods) % 3 != 0:
            raise MpnhipError("forward_native: fc must be (Linear, BatchNorm1d, ReLU) triples")
        triples = []
        for i in range(0, len(mods), 3):
            lin, bn, act = mods[i:i + 3]
            if not (isinstance(lin, nn.Linear) and isinstance(bn, nn.BatchNorm1d) and isinstance(act, nn.ReLU)):
                raise MpnhipError("forward_native: fc must be (Linear, BatchNorm1d, ReLU) triples")
            triples.append((lin, bn))
        return triples

    def _check_native(self):
        if self.training:
            raise MpnhipError("forward_native is the inference forward (eval-mode BatchNorm): call .eval() first")
        if self.dropout_p is not None:
            raise MpnhipError("forward_native does not cover dropout_p")
        if self.block is not Bottleneck:
            raise MpnhipError("forward_native covers Bottleneck blocks only, not %s" % getattr(self.block, "__name__", self.block))

    def prepare_native(self):
        """Folds every BatchNorm: ``self._native = {'affine': {conv name: (scale, shift)}, 'fc': [(weight, bias), ...], 'plans':
        {(H, W): launch list}}`` on the parameters' device.  Called by ``forward_native`` when no cache exists."""
        self._check_native()
        mods = dict(self.named_modules())
        affine = OrderedDict((c["name"], fold_batchnorm(mods[c["bn"]])) for c in self.conv_layers(128, 64))
        fc = [fold_linear_batchnorm(lin, bn) for lin, bn in self._fc_triples()]
        self._native = dict(affine=affine, fc=fc, plans={})
        return self._native

    def _plan(self, native, H, W):
        """The launch list of one slice for an ``H x W`` input, cached beside the folded constants: the convolutions in execution
        order with their weights and constants and the buffers they read and write.  Buffers: 'x' the input, 0 .. 2 the three
        activation buffers the blocks take turns in, 'f' the result.  Inside a bottleneck with its input in buffer ``ci`` and
        ``a``, ``b`` the other two: conv1 -> a, conv2 -> b; without a downsample conv3 reads b, adds ci and writes a (conv1's
        output is dead); with one the shortcut goes to a and conv3 reads b, adds a and writes ci (the input is dead) -- an output
        never overlaps what its launch reads."""
        plan = native["plans"].get((H, W))
        if plan is not None:
            return plan
        mods = dict(self.named_modules())
        layers = {c["name"]: c for c in self.conv_layers(H, W)}
        for name, c in layers.items():
            c["weight"] = mods[name].weight                 # the parameter itself: a deepcopy of the module keeps the tie
            if not c["weight"].is_contiguous():
                raise MpnhipError("forward_native: %s.weight is not contiguous" % name)
            c["scale"], c["shift"] = native["affine"][name]
            c["floats"] = c["cout"] * c["Hout"] * c["Wout"]
        names = list(layers)
        steps = [("conv", layers["conv1"], 'x', 0, None, True), ("pool", layers["conv1"], 0, 1, None, False), ("stage", "stem", 1)]
        ci = 1
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(self, "layer%d" % li)):
                p = "layer%d.%d." % (li, bi)
                a, b = [i for i in range(3) if i != ci]
                last = p + "conv3" == names[-1]
                steps.append(("conv", layers[p + "conv1"], ci, a, None, True))
                steps.append(("conv", layers[p + "conv2"], a, b, None, True))
                if blk.downsample is None:
                    steps.append(("conv", layers[p + "conv3"], b, 'f' if last else a, ci, True))
                    ci = a
                else:
                    steps.append(("conv", layers[p + "downsample.0"], ci, a, None, False))
                    steps.append(("conv", layers[p + "conv3"], b, 'f' if last else ci, a, True))
            steps.append(("stage", "layer%d" % li, 'f' if li == 4 else ci))
        final = layers[names[-1]]
        plan = dict(steps=steps, per_image=max(c["floats"] for c in layers.values()), final=final)
        native["plans"][(H, W)] = plan
        return plan

    @torch.no_grad()
    def forward_native(self, x, max_images=1000, stages=None):
        """``forward`` without autograd through the native kernels: ``(f, v)``.  ``x``: float32 ``[n, 3, H, W]`` on the device.
        The batch is processed in slices of at most ``max_images`` (and never more than ``MAX_SLICE``), so the largest activation
        stays within 32-bit offsets and ``v``'s bits do not depend on the batch; the
        activations of a slice live in three buffers from the torch allocator that the blocks take turns in.  ``stages``
        (diagnosis): a list that receives ``(name, copy)`` of the activation after the stem (``'stem'``: conv1, bn1, ReLU,
        max-pool) and after ``'layer1'`` .. ``'layer4'``, per slice."""
        self._check_native()
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise MpnhipError("forward_native takes a float32 [n, 3, H, W] tensor on the device")
        if self.conv1.weight.device != x.device or self.conv1.weight.dtype != torch.float32:
            raise MpnhipError("forward_native: the module must be float32 on the input's device (%s)" % x.device)
        native = self._native if self._native is not None else self.prepare_native()
        x = _dense_input(x, "x")
        n, _, H, W = (int(s) for s in x.shape)
        plan = self._plan(native, H, W)
        step = max(min(int(max_images), n, MAX_SLICE), 1)
        final = plan["final"]
        hf, wf, cf = final["Hout"], final["Wout"], final["cout"]
        lib = capi.load()
        args = capi.ConvAffineArgs()
        with torch.cuda.device(x.device):
            stream = capi.stream_ptr()
            f = torch.empty((n, cf, hf, wf), dtype=torch.float32, device=x.device)
            v = torch.empty((n, self.feature_dim), dtype=torch.float32, device=x.device)
            bufs = [torch.empty(step * plan["per_image"], dtype=torch.float32, device=x.device) for _ in range(3)]
            for k0 in range(0, n, step):
                m = min(step, n - k0)
                # buffer -> [address, floats per image, shape of an image] of what it holds now
                held = {'x': [x[k0:k0 + m].data_ptr(), x.stride(0), None], 'f': [f[k0:k0 + m].data_ptr(), f.stride(0), (cf, hf, wf)]}
                for i in range(3):
                    held[i] = [bufs[i].data_ptr(), 0, None]
                for st in plan["steps"]:
                    if st[0] == "stage":
                        if stages is not None:
                            src = f[k0:k0 + m] if st[2] == 'f' else bufs[st[2]][:m * held[st[2]][1]].view((m,) + held[st[2]][2])
                            stages.append((st[1], src.clone()))
                        continue
                    kind, c, src, dst, res, relu = st
                    if kind == "pool":
                        hp, wp = _conv_out(c["Hout"], 2), _conv_out(c["Wout"], 2)
                        held[dst][1:] = [c["cout"] * hp * wp, (c["cout"], hp, wp)]
                        capi.check(lib.mpnhip_maxpool2d_forward(held[src][0], held[src][1], m, c["cout"], c["Hout"], c["Wout"], held[dst][0],
                                                                held[dst][1], stream), "mpnhip_maxpool2d_forward")
                        continue
                    if dst != 'f':
                        held[dst][1:] = [c["floats"], (c["cout"], c["Hout"], c["Wout"])]
                    args.x, args.x_stride, args.weight = held[src][0], held[src][1], c["weight"].data_ptr()
                    args.scale, args.shift = c["scale"].data_ptr(), c["shift"].data_ptr()
                    args.residual, args.residual_stride = (held[res][0], held[res][1]) if res is not None else (None, 0)
                    args.relu, args.out, args.out_stride, args.n_images = int(relu), held[dst][0], held[dst][1], m
                    args.cin, args.cout, args.H, args.W, args.ksize, args.stride = c["cin"], c["cout"], c["H"], c["W"], c["k"], c["stride"]
                    capi.check(lib.mpnhip_conv2d_affine_forward(C.byref(args), stream), "mpnhip_conv2d_affine_forward")
                pooled = torch.empty((m, cf), dtype=torch.float32, device=x.device)
                capi.check(lib.mpnhip_avgpool(held['f'][0], m * cf, hf * wf, capi.ptr(pooled), stream), "mpnhip_avgpool")
                h = pooled
                for i, (wt, bias) in enumerate(native["fc"]):
                    y = v[k0:k0 + m] if i == len(native["fc"]) - 1 else torch.empty((m, wt.shape[0]), dtype=torch.float32, device=x.device)
                    capi.check(lib.mpnhip_linear(capi.ptr(h), h.stride(0), capi.ptr(wt), capi.ptr(bias), capi.ptr(y), y.stride(0), m,
                                                 int(wt.shape[0]), int(wt.shape[1]), 1, stream), "mpnhip_linear")
                    h = y
                if not native["fc"]:
                    v[k0:k0 + m].copy_(pooled)
        return f, v


def resnet50_fc256(num_classes, loss='xent'):
    """The reference's ReID network (``resnet.py:453-466``): ResNet50 with last stride 1 and ``fc`` = 2048 -> 1024 -> 256."""
    return ResNet(num_classes=num_classes, loss=loss, block=Bottleneck, layers=[3, 4, 6, 3], last_stride=1, fc_dims=[1024, 256],
                  dropout_p=None)


def load_pretrained_weights(model, weight_path):
    """Loads a checkpoint file into ``model`` with the reference loader's tolerance: a ``{'state_dict': ...}`` wrapper is opened,
    a ``module.`` prefix (DataParallel) is stripped, keys whose name or size does not match are skipped.  Returns
    ``(loaded keys, skipped keys)``."""
    ckpt = torch.load(weight_path, map_location="cpu")
    state = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
    own = model.state_dict()
    loaded, skipped = [], []
    for k, t in state.items():
        if k.startswith("module."):
            k = k[len("module."):]
        if k in own and isinstance(t, torch.Tensor) and own[k].size() == t.size():
            own[k] = t
            loaded.append(k)
        else:
            skipped.append(k)
    model.load_state_dict(own)
    return loaded, skipped
