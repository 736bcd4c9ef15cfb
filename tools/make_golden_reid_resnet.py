#!/usr/bin/env python3
"""Generate tests/golden/g26_reid_resnet.npz by running the REFERENCE's ReID network (authoring container only).

The reference's Python never travels to the GPU box; this script loads ``models/resnet.py`` from the reference checkout by file
path, builds ``resnet50_fc256(10, loss='xent', pretrained=False)`` -- never with ``pretrained=True``, its default, which would go
to ``model_zoo.load_url`` --, fills it with ``synth.make_reid_weights``, and runs it in float64 on the CPU on
``synth.normal(seed, (3, 3, 128, 64), stream=synth.REID_INPUT_STREAM)``.  Stored: the ordered ``state_dict`` names and shapes, v in
float64, f in float64 at every 8th element with f's sum and abs-sum, and the seed.  Nothing of the reference's text is stored.

    python tools/make_golden_reid_resnet.py [--reference /root/reference] [--seed 31]
"""
import sys

sys.dont_write_bytecode = True

import argparse
import importlib.util
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mpntrackseg_amd import synth  # noqa: E402

F_SAMPLE_STEP = 8


def load_reference_resnet(reference):
    path = os.path.join(reference, "src", "mot_neural_solver", "models", "resnet.py")
    spec = importlib.util.spec_from_file_location("reference_reid_resnet", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "g26_reid_resnet.npz"))
    args = ap.parse_args()

    ref = load_reference_resnet(args.reference)
    net = ref.resnet50_fc256(10, loss='xent', pretrained=False)
    synth.make_reid_weights(net, args.seed)
    net = net.eval().double()
    sd = net.state_dict()
    x = torch.from_numpy(synth.normal(args.seed, (3, 3, 128, 64), stream=synth.REID_INPUT_STREAM)).double()
    with torch.no_grad():
        f, v = net(x)
    f = f.numpy().reshape(-1)
    names = list(sd)
    shapes = np.full((len(names), 4), -1, np.int64)
    for i, k in enumerate(names):
        shapes[i, :sd[k].dim()] = list(sd[k].shape)
    np.savez_compressed(args.out, seed=np.int64(args.seed), names=np.array(names), shapes=shapes, v=v.numpy(),
                        f_shape=np.array([3, 2048, 8, 4], np.int64), f_step=np.int64(F_SAMPLE_STEP), f_sample=f[::F_SAMPLE_STEP].copy(),
                        f_sum=np.float64(f.sum()), f_abs_sum=np.float64(np.abs(f).sum()), f_zero_share=np.float64((f == 0).mean()),
                        v_zero_share=np.float64((v.numpy() == 0).mean()))
    print("wrote %s: %d entries, max |f| %.4g, max |v| %.4g, zeros f %.3f v %.3f, %d bytes"
          % (args.out, len(names), np.abs(f).max(), v.abs().max(), (f == 0).mean(), (v.numpy() == 0).mean(), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
