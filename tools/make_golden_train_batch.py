#!/usr/bin/env python3
"""Generate tests/golden/g25_train_samples.npz by running the REFERENCE's training sampler (authoring container only):
``MOTGraphDataset._compute_seq_step_sizes`` / ``_index_dataset`` / ``get_from_frame_and_seq`` (data/mot_graph_dataset.py),
``MOTGraph._construct_graph_df`` / ``construct_graph_object`` / ``assign_edge_labels`` (data/mot_graph.py) and
``MOTGraphAugmentor`` (data/augmentation.py), imported from the reference tree, on two synthetic sequences.

The dataset object is built without its ``__init__`` (which reads detection files): the attributes the methods read are set
by hand, the ``object.__new__`` technique of ``make_golden.gen_g14``.  ``MOTGraph._load_appearance_data`` and
``assign_mask_labels``, which read embedding files, are replaced by lookups into tensors by ``detection_id``.  numpy's global
generator is only OBSERVED (the outputs of ``uniform`` and the sizes of ``choice`` are noted down), never changed.

Usage:  python tools/make_golden_train_batch.py
"""
import sys
sys.dont_write_bytecode = True  # never leave __pycache__ inside the read-only reference tree
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import make_golden as MK  # noqa: E402
from mpntrackseg_amd import synth  # noqa: E402

BOX_COLS = ("bb_left", "bb_top", "bb_right", "bb_bot", "bb_width", "bb_height", "feet_x", "feet_y")
EDGE_FEATS = ["secs_time_dists", "norm_feet_x_dists", "norm_feet_y_dists", "bb_height_dists", "bb_width_dists", "emb_dist"]
DATASET_PARAMS = {
    "frames_per_graph": 6, "max_detects": 16, "min_detects": 4, "max_frame_dist": 4, "top_k_nns": 3, "reciprocal_k_nns": True,
    "edge_feats_to_use": EDGE_FEATS, "true_edge_labels": "closest", "augment": True, "p_change_fps_step": 0.5,
    "min_ids_to_drop_perc": 0.0, "max_ids_to_drop_perc": 0.3, "min_detects_to_drop_perc": 0.0, "max_detects_to_drop_perc": 0.3,
    "min_iou_bb_wiggling": 0.85, "target_fps_dict": {"moving": 9, "static": 6},
}
# detections per frame (frames 1, 2, ...): empty frames, a run of single detections (frames 7-10 of A)
COUNTS = {
    "A": [3, 4, 0, 5, 2, 6, 1, 1, 1, 1, 0, 0, 4, 5, 3, 6, 2, 4, 0, 3, 5, 4, 6, 2, 3, 1, 4, 5, 0, 3, 2, 4, 3, 2, 0, 1, 2, 3, 2, 1],
    "B": [2, 3, 1, 4, 0, 2, 3, 3, 1, 2, 4, 2, 0, 3, 2, 1],
}
INFO = {"A": {"fps": 20, "mov_camera": False}, "B": {"fps": 6, "mov_camera": False}}
UNTRACKED_FROM = {"A": 31, "B": 10 ** 9}    # from this frame on every detection of the sequence has id -1


def make_sequence(name, seed):
    import pandas as pd
    counts = np.asarray(COUNTS[name], np.int64)
    frame = np.repeat(np.arange(1, counts.size + 1, dtype=np.int64), counts)
    n = frame.size
    rs = np.random.RandomState(seed)
    ids = np.empty(n, np.int64)
    for f in np.unique(frame):
        sel = np.nonzero(frame == f)[0]
        pool = (np.arange(sel.size) + f // 5) % 7 + 1                # distinct track ids inside a frame, lasting a few frames ...
        pool = np.where(rs.rand(sel.size) < 0.25, -1, pool)          # ... and unmatched detections
        ids[sel] = -1 if f >= UNTRACKED_FROM[name] else pool
    w = 30.0 + 60.0 * rs.rand(n)
    h = 80.0 + 120.0 * rs.rand(n)
    left = 1800.0 * rs.rand(n)
    top = 100.0 + 700.0 * rs.rand(n)
    df = pd.DataFrame({"frame": frame, "detection_id": np.arange(n, dtype=np.int64), "id": ids, "bb_left": left, "bb_top": top,
                       "bb_width": w, "bb_height": h, "bb_right": left + w, "bb_bot": top + h, "feet_x": left + 0.5 * w,
                       "feet_y": top + h})
    df["frame_path"] = "synthetic/img1/000001.jpg"
    # shuffled rows: _construct_graph_df has to sort them (mot_graph.py:145)
    df = df.iloc[rs.permutation(n)].reset_index(drop=True)
    return df, synth.normal(seed, (n, 32), stream=6), synth.normal(seed, (n, 64), stream=7)


class Watch:
    """Notes what numpy's global generator hands out while a reference sample is drawn."""

    def __enter__(self):
        self.uniforms, self.choices = [], []
        self.real = (np.random.uniform, np.random.choice)

        def uniform(*a, **k):
            out = self.real[0](*a, **k)
            self.uniforms.append(np.array(out, np.float64))
            return out

        def choice(a, size=None, replace=True, p=None):
            out = self.real[1](a, size, replace, p)
            self.choices.append(np.array(out))
            return out
        np.random.uniform, np.random.choice = uniform, choice
        return self

    def __exit__(self, *exc):
        np.random.uniform, np.random.choice = self.real


def main():
    MK._import_tracking_stack()
    # the stack above parks stand-ins where the sampler's modules go: take them out and import the real ones.  The sequence
    # processor (detection files, CNNs) is unrelated to the methods under test and needs yet more packages
    for name in ("mot_neural_solver.data.augmentation", "mot_neural_solver.data.mot_graph_dataset"):
        del sys.modules[name]
    MK._placeholder_modules([("mot_neural_solver.data.seq_processing", []),
                             ("mot_neural_solver.data.seq_processing.seq_processor", ["MOTSeqProcessor"])])
    from mot_neural_solver.data import augmentation as AUG
    from mot_neural_solver.data import mot_graph as MG
    from mot_neural_solver.data import mot_graph_dataset as DS
    from mot_neural_solver.utils.iou import iou_pairs
    MG.MOTGraphAugmentor = AUG.MOTGraphAugmentor    # (mot_graph.py bound the stand-in at import)
    MG.scatter_min = MK._real_scatter_min

    seqs = {"A": make_sequence("A", 31), "B": make_sequence("B", 32)}
    names = list(seqs)

    def appearance(self):
        _, reid, x = seqs[self.seq_info_dict["name"]]
        rows = self.graph_df.detection_id.values
        return torch.from_numpy(reid[rows]), torch.from_numpy(x[rows]).view(-1, 64, 1, 1), None
    MG.MOTGraph._load_appearance_data = appearance
    MG.MOTGraph.assign_mask_labels = lambda self: None

    def dataset(mode, **change):
        ds = object.__new__(DS.MOTGraphDataset)
        ds.dataset_params = dict(DATASET_PARAMS, **change)
        ds.mode = mode
        ds.augment = ds.dataset_params["augment"] and mode == "train"
        ds.seq_det_dfs = {n: seqs[n][0] for n in names}
        ds.seq_info_dicts = {n: dict(INFO[n], name=n) for n in names}
        ds.seq_names = names
        ds._compute_seq_step_sizes()
        return ds

    rec = {}
    ds = dataset("train")
    for n in names:
        df, reid, x = seqs[n]
        for c in ("frame", "detection_id", "id") + BOX_COLS:
            rec[f"{n}:{c}"] = df[c].values
        rec[f"{n}:reid"], rec[f"{n}:x"] = reid, x
        rec[f"{n}:info"] = np.array([INFO[n]["fps"], int(INFO[n]["mov_camera"]), ds.seq_info_dicts[n]["step_size"]], np.int64)
    assert ds.seq_info_dicts["A"]["step_size"] == 3 and ds.seq_info_dicts["B"]["step_size"] == 1
    for k in ("frames_per_graph", "max_detects", "min_detects", "max_frame_dist", "top_k_nns", "reciprocal_k_nns"):
        rec[f"params:{k}"] = np.int64(DATASET_PARAMS[k])
    for k in ("p_change_fps_step", "min_ids_to_drop_perc", "max_ids_to_drop_perc", "min_detects_to_drop_perc",
              "max_detects_to_drop_perc", "min_iou_bb_wiggling"):
        rec[f"params:{k}"] = np.float64(DATASET_PARAMS[k])
    rec["params:target_fps"] = np.array([DATASET_PARAMS["target_fps_dict"]["moving"], DATASET_PARAMS["target_fps_dict"]["static"]], np.int64)

    # ---- _compute_seq_step_sizes on more rates (a tie that Python's round takes to the even side among them)
    steps = []
    for fps, mov in ((15, False), (21, False), (30, True), (6, False), (9, True), (25, True), (27, False)):
        probe = object.__new__(DS.MOTGraphDataset)
        probe.dataset_params = DATASET_PARAMS
        probe.seq_info_dicts = {"p": {"fps": fps, "mov_camera": mov}}
        probe._compute_seq_step_sizes()
        steps.append((fps, int(mov), probe.seq_info_dicts["p"]["step_size"]))
    rec["step_sizes"] = np.array(steps, np.int64)

    # ---- _index_dataset
    for n in names:
        for step, fpg, mind in ((1, 5, 4), (3, 5, 8), (2, 15, 25), (3, 6, 4), (1, 6, 4)):
            d = dataset("train", frames_per_graph=fpg, min_detects=mind)
            d.seq_det_dfs = {n: seqs[n][0]}
            d.seq_info_dicts[n]["step_size"] = step
            got = np.array([f for _, f in d._index_dataset()], np.int64)
            rec[f"index:{n}:{step}_{fpg}_{mind}"] = got
            print("g25 index", n, (step, fpg, mind), got.size, "start frames")
    assert rec["index:A:2_15_25"].size < 12 and rec["index:B:2_15_25"].size == 0     # few, and none

    # ---- _construct_graph_df: (sequence, start, step, frames_per_graph or -1 = 'max', max_detects or -1 = None, end_frame or -1, ensure)
    windows = {"fpg_cut": ("A", 4, 3, 4, -1, -1, 0), "max_detects_cut": ("A", 13, 1, 8, 14, -1, 0), "both": ("A", 1, 3, 6, 16, -1, 0),
               "fpg_max": ("A", 22, 3, -1, -1, -1, 0), "end": ("A", 5, 3, 6, 16, 18, 0), "end_ensure": ("A", 5, 3, 6, 16, 18, 1),
               "end_ensure_hit": ("A", 5, 3, 6, 16, 17, 1), "tail_one_frame": ("A", 39, 3, 6, 16, -1, 0), "tail_empty": ("A", 40, 3, 6, 16, -1, 0),
               "starts_on_empty": ("A", 3, 1, 6, 16, -1, 0), "B_step1": ("B", 2, 1, 6, 16, -1, 0), "B_tail": ("B", 14, 2, 6, 16, -1, 0)}
    for tag, (n, start, step, fpg, maxd, end, ensure) in windows.items():
        mg = object.__new__(MG.MOTGraph)
        mg.dataset_params = dict(DATASET_PARAMS, frames_per_graph="max" if fpg < 0 else fpg, max_detects=None if maxd < 0 else maxd)
        mg.step_size = step
        gdf, frames = mg._construct_graph_df(seqs[n][0].copy(), start, None if end < 0 else end, bool(ensure))
        rec[f"rows:{tag}:args"] = np.array([names.index(n), start, step, fpg, maxd, end, ensure], np.int64)
        rec[f"rows:{tag}:detection_id"] = gdf.detection_id.values.astype(np.int64)
        print("g25 rows", tag, len(gdf), "rows, frames", frames)
    assert rec["rows:tail_empty:detection_id"].size == 0 and len(np.unique(seqs["A"][0].frame.values[
        np.isin(seqs["A"][0].detection_id.values, rec["rows:tail_one_frame:detection_id"])])) == 1
    assert rec["rows:end_ensure:detection_id"].size > rec["rows:end:detection_id"].size

    # ---- whole samples: get_from_frame_and_seq(mode 'train', augment on) for (seed, sequence, start_frame), then two 'val' samples
    def run(d, seed, n, start):
        np.random.seed(seed)
        with Watch() as w:
            mg = d.get_from_frame_and_seq(seq_name=n, start_frame=start, max_frame_dist=d.dataset_params["max_frame_dist"],
                                          return_full_object=True, inference_mode=False)
        return mg, w, np.random.rand()

    def search(d, n, start, want):
        for seed in range(200):
            mg, w, nxt = run(d, seed, n, start)
            if want(mg, w):
                return seed, mg, w, nxt
        raise SystemExit("no seed gives the wanted sample")

    plans = [("A", 1, lambda mg, w: mg.step_size == 3 and w.choices[0].size > 0 and w.choices[1].size > 0),
             ("A", 13, lambda mg, w: mg.step_size == 2),                     # the step change is drawn and takes effect
             ("A", 20, lambda mg, w: w.choices[0].size == 0),                # drops no id
             ("A", 31, lambda mg, w: True),                                  # no id other than -1
             ("B", 2, lambda mg, w: w.choices[1].size > 0),
             ("B", 8, lambda mg, w: w.choices[0].size > 0)]
    train, val = dataset("train"), dataset("val")
    samples = [search(train, n, start, want) + (n, start, 1) for n, start, want in plans]
    samples += [(0,) + run(val, 0, "A", 4) + ("A", 4, 0), (0,) + run(val, 0, "B", 5) + ("B", 5, 0)]
    for k, (seed, mg, w, nxt, n, start, is_train) in enumerate(samples):
        g, df0 = mg.graph_df, seqs[n][0].set_index("detection_id")
        rec[f"s{k}:args"] = np.array([seed, names.index(n), start, is_train], np.int64)
        rec[f"s{k}:step_size"] = np.int64(mg.step_size)
        rec[f"s{k}:next_rand"] = np.float64(nxt)
        for c in ("frame", "detection_id", "id"):
            rec[f"s{k}:{c}"] = g[c].values.astype(np.int64)
        for c in BOX_COLS:
            rec[f"s{k}:{c}"] = g[c].values.astype(np.float64)
        go = mg.graph_obj
        rec[f"s{k}:edge_index"], rec[f"s{k}:edge_attr"] = go.edge_index.numpy(), go.edge_attr.numpy()
        rec[f"s{k}:edge_labels"] = go.edge_labels.numpy().astype(np.float32)
        if is_train:
            rec[f"s{k}:eps"] = w.uniforms[-1].reshape(-1, 4)
            assert len(w.uniforms) == 3 and len(w.choices) == 2 and rec[f"s{k}:eps"].shape[0] == len(g)
            # the reference's own assertion (augmentation.py:86) held -- it ran -- and here it is once more on the stored numbers
            orig = df0.loc[g.detection_id.values]
            cols = ["bb_left", "bb_top", "bb_right", "bb_bot"]
            iou = iou_pairs(g[cols].values.T, orig[cols].values.T)
            assert iou.min() >= DATASET_PARAMS["min_iou_bb_wiggling"], iou.min()
            rec[f"s{k}:min_iou"] = np.float64(iou.min())
        else:
            assert not w.uniforms and not w.choices
        print("g25 sample", k, n, "seed", seed, "start", start, "train" if is_train else "val", "step", mg.step_size, "nodes", len(g),
              "edges", go.edge_index.shape[1], "positives", int(go.edge_labels.sum()))
    assert set(rec["s3:id"].tolist()) == {-1} and rec["s1:step_size"] == 2
    for k in range(len(samples)):   # the pruning removes edges at this size
        assert rec[f"s{k}:edge_index"].shape[1] > 0
    out = os.path.join(MK.GOLD, "g25_train_samples.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
