"""Child program of tests/test_gpu_joint_train_distributed.py (launched with torch.distributed.run; 2 ranks on gloo, both on cuda:0, or
1 rank on nccl): the data-parallel JOINT step -- TrainStep(train_mask_branch=True), each rank its own graph.  The averaged flat
gradient (mask segment included) is the mean of the two single-rank joint gradients, both ranks hold identical parameters after
Adam, an invalid graph on one rank stops every rank's optimizer step (mask branch included), and a 1-rank RCCL group with
force_collectives gives the plain joint step."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch
import torch.distributed as dist

import joint_train_common as J
from mpntrackseg_amd import capi
from mpntrackseg_amd.train import TrainStep


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    what = sys.argv[1] if len(sys.argv) > 1 else "average"
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    torch.cuda.set_device(0)
    p = J.model_params(num_class_steps=2, L=L)
    if what == "nccl1":
        dist.init_process_group("nccl", device_id=J.DEV)
        return nccl_one_rank_check(p, L)
    dist.init_process_group("gloo")
    if what == "badgraph":
        return bad_graph_check(rank, world, p)
    batches = [J.device_batch("A"), J.device_batch("B")]
    # the single-rank joint gradient of every graph (no collective, no optimizer step), each computed by the rank that owns the graph
    # and then gathered: the stock convolutions' backward algorithms are chosen per process (the library times its candidates), and
    # two algorithms differ by more than two routes to one gradient do -- every graph's gradient must come from ONE process
    st = TrainStep(J.fresh(p), world_size=1, train_mask_branch=True)
    st.batch(batches[rank], optimizer_step=False)
    torch.cuda.synchronize()
    own = st.bucket.flat[:st.bucket.n].detach().clone()
    singles = [torch.zeros_like(own) for _ in range(world)]
    dist.all_gather(singles, own)
    want = sum(s.double().cpu().numpy() for s in singles) / world
    step = TrainStep(J.fresh(p), world_size=world, lr=1e-3, train_mask_branch=True)
    start = step.bucket.flat_params.detach().clone()
    step.batch(batches[rank])
    torch.cuda.synchronize()
    got = step.bucket.flat.double().cpu().numpy()
    err = J.rel(got[:step.bucket.n], want)
    err_mask = J.rel(got[:step.mask_elems], want[:step.mask_elems])
    flag = float(np.abs(got[step.bucket.n:]).max())
    uses_side = bool(capi.load().mpnhip_backward_uses_side_stream(step.model.c_model([])))
    mine = step.bucket.flat_params.detach().clone()
    gathered = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(gathered, mine)
    same = all(torch.equal(gathered[0], t) for t in gathered[1:])
    moved_mask = not torch.equal(mine[:step.mask_elems], start[:step.mask_elems])
    moved_hot = not torch.equal(mine[step.mask_elems:], start[step.mask_elems:])
    print("RANK %d joint err %.3e mask %.3e flag %.1f side_stream %d same_params %d moved %d %d applied %d"
          % (rank, err, err_mask, flag, uses_side, same, moved_mask, moved_hot, step.opt.applied_steps), flush=True)
    ok = err < 2e-5 and err_mask < 2e-5 and flag == 0.0 and same and moved_mask and moved_hot and uses_side == (L >= 4) \
        and step.opt.applied_steps == 1
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 3)


def bad_graph_check(rank, world, p):
    """Rank 1's edge_index leaves [0, N): it raises IndexError AFTER taking part in all the step's collectives (the mask segment's
    early one included), and NO rank applies the optimizer step -- the mask branch's parameters stay as they were too."""
    b = dict(J.device_batch("A" if rank == 0 else "B"))
    if rank == 1:
        ei = b["edge_index"].clone()
        ei[1, 7] = b["x"].shape[0]   # one past the last node
        b["edge_index"] = ei
    step = TrainStep(J.fresh(p), world_size=world, lr=1e-2, train_mask_branch=True)
    before = step.bucket.flat_params.detach().clone()
    raised = False
    try:
        step.batch(b)
    except IndexError:
        raised = True
    torch.cuda.synchronize()
    unchanged = bool(torch.equal(before, step.bucket.flat_params))
    applied = step.opt.applied_steps
    print("RANK %d joint badgraph raised %d unchanged %d applied %d" % (rank, raised, unchanged, applied), flush=True)
    ok = unchanged and raised == (rank == 1) and applied == 0 and step.opt.t == 1
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 5)


def nccl_one_rank_check(p, L):
    """force_collectives on a 1-rank RCCL group: the mask segment's asynchronous all-reduce behind the autograd pass, the
    message-passing bucket's on the library's side stream, the encoder's on the caller's stream -- all issued, all waited for --
    then / 1 and the guarded Adam: the plain joint step's gradients and parameters within the 1e-5 of the hot-path-only check."""
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    b = J.device_batch("AB")
    plain = TrainStep(J.fresh(p), world_size=1, lr=1e-3, train_mask_branch=True)
    coll = TrainStep(J.fresh(p), world_size=1, lr=1e-3, train_mask_branch=True, force_collectives=True)
    issued = []
    inner = coll.allreduce_mask_segment

    def counted():
        w = inner()
        issued.append(w is not None)
        return w
    coll.allreduce_mask_segment = counted
    ok = True
    for it in range(2):
        plain.batch(b)
        coll.batch(b)
        torch.cuda.synchronize()
        dg = J.rel(coll.bucket.flat[:coll.bucket.n].double().cpu().numpy(), plain.bucket.flat[:plain.bucket.n].double().cpu().numpy())
        dp = J.rel(coll.bucket.flat_params.double().cpu().numpy(), plain.bucket.flat_params.double().cpu().numpy())
        side = L >= 4 and hasattr(coll, "ev_mp_ready")
        print("NCCL1 joint step %d grad diff %.2e param diff %.2e side %d applied %d" % (it, dg, dp, side, coll.opt.applied_steps), flush=True)
        # the parameters are compared after the FIRST step only: the two runs' gradients differ in summation order (1e-8), and Adam
        # divides by sqrt(v) + eps -- an element whose gradient is of the size of that difference moves by up to lr either way, so
        # from the second step on the parameters of the two runs are not within 1e-5 although every gradient still is
        ok = ok and dg < 1e-5 and (dp < 1e-5 or it > 0) and coll.opt.applied_steps == it + 1 and side == (L >= 4)
    ok = ok and issued == [True, True]
    print("NCCL1 joint ok %d mask_collectives %d" % (ok, len(issued)), flush=True)
    dist.destroy_process_group()
    sys.exit(0 if ok else 6)


if __name__ == "__main__":
    main()
