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
from collections import OrderedDict

import torch
from torch import nn

from . import capi
from .capi import MpnhipError
from .conv_affine import (Bottleneck, DropsNativeCache, _Held, _dense_input, bind_layer, fold_batchnorm, fold_linear_batchnorm,
                          make_layer, resnet_body_steps, resnet_conv_layers, run_steps)
from .conv_affine import conv2d_affine_native, maxpool2d_native  # noqa: F401  (importable from here as before)


MAX_SLICE = 8191      # crops per slice of forward_native: launch_gemm changes its kernel (hence v's summation) at 8192 rows


class ResNet(DropsNativeCache, nn.Module):
    """``models/resnet.py``'s ResNet for the block types this project runs (``Bottleneck``), see the module docstring."""

    def __init__(self, num_classes, loss, block, layers, last_stride=2, fc_dims=None, dropout_p=None):
        super().__init__()
        self.loss = loss
        self.block = block
        self.dropout_p = dropout_p
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = make_layer(block, 64, 64, layers[0], 1)
        self.layer2 = make_layer(block, 64 * block.expansion, 128, layers[1], 2)
        self.layer3 = make_layer(block, 128 * block.expansion, 256, layers[2], 2)
        self.layer4 = make_layer(block, 256 * block.expansion, 512, layers[3], last_stride)
        self.global_avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.feature_dim = 512 * block.expansion
        self.fc = self._construct_fc_layer(fc_dims, 512 * block.expansion, dropout_p)
        self.classifier = nn.Linear(self.feature_dim, num_classes)
        self._native = None
        self._init_params()

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

    # ---- the native forward
    def conv_layers(self, H, W):
        """Every convolution of ``featuremaps`` in execution order for an ``H x W`` input (``conv_affine.resnet_conv_layers``)"""
        return resnet_conv_layers(self, "", H, W)

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
        order with their weights and constants and the buffers they read and write (``conv_affine.resnet_body_steps``): 'x' the
        input, 0 .. 2 the three activation buffers the blocks take turns in, 'f' -- the result -- kept from layer4."""
        plan = native["plans"].get((H, W))
        if plan is not None:
            return plan
        mods = dict(self.named_modules())
        layers = {c["name"]: bind_layer(c, mods[c["name"]], *native["affine"][c["name"]]) for c in self.conv_layers(H, W)}
        steps = resnet_body_steps(self, "", layers, {4: 'f'}, ("layer1", "layer2", "layer3", "layer4"))
        plan = dict(steps=steps, per_image=max(c["floats"] for c in layers.values()), final=list(layers.values())[-1])
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
        cf, hf, wf = plan["final"]["out_shape"]
        lib = capi.load()
        with torch.cuda.device(x.device):
            stream = capi.stream_ptr()
            f = torch.empty((n, cf, hf, wf), dtype=torch.float32, device=x.device)
            v = torch.empty((n, self.feature_dim), dtype=torch.float32, device=x.device)
            bufs = [torch.empty(step * plan["per_image"], dtype=torch.float32, device=x.device) for _ in range(3)]
            for k0 in range(0, n, step):
                m = min(step, n - k0)
                fs = f[k0:k0 + m]
                held = {'x': _Held(x[k0:k0 + m].data_ptr(), x.stride(0), (3, H, W), fixed=True),
                        'f': _Held(fs.data_ptr(), f.stride(0), (cf, hf, wf), fixed=True, tensor=fs.view(-1) if stages is not None else None)}
                for i in range(3):
                    held[i] = _Held(bufs[i].data_ptr(), tensor=bufs[i])
                run_steps(plan["steps"], held, m, lib, stream, stages)
                pooled = torch.empty((m, cf), dtype=torch.float32, device=x.device)
                capi.check(lib.mpnhip_avgpool(held['f'].address, m * cf, hf * wf, capi.ptr(pooled), stream), "mpnhip_avgpool")
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
