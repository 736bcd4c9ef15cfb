"""Data-parallel training step: one graph per GPU, flat gradient buckets, RCCL all-reduce overlapped with the backward.

The reference trains on one GPU with ``accumulate_grad_batches: 8`` (configs/tracking_cfg.yaml:4,
scripts/train.py:76); W GPUs x 1 graph with gradient averaging is the same optimisation step executed
in space instead of time.  The graphs share nothing but the weights, so the
data path has no collective; the only exchange is the all-reduce(sum) / W of the flat fp32 gradient buffer
per optimizer step (1.2 MB at the reference dims, 19 MB at d = 128), issued as two buckets: the gradients of the
message-passing modules and the classifier are final when the backward's last weight-gradient group is (on the
library's side stream) -- their all-reduce starts there and runs under the encoder's backward; the encoder's bucket
follows on the caller's stream.

``TrainStep(train_mask_branch=True)`` is the reference's joint step (pl_module.py:88-135): the mask branch's parameters share the
flat bucket, its loss reaches every step's logits, and a third all-reduce (the mask segment, issued first) runs beside the native
backward.  ``TrainStep.evaluate`` is the validation step, ``EpochLog`` the epoch's log on the device, ``state_dict`` /
``load_state_dict`` checkpoint and resume."""
import torch

from . import capi
from .autograd import native_backward, native_forward_saved


def backward_available():
    """True when libmpnhip.so carries the hand-written backward."""
    lib = capi.load()
    return lib.mpnhip_backward_workspace_bytes(None, 0, 0) != 0


def shard_indices(n_items, rank, world_size):
    """Round-robin shard of sample (graph / sequence) ids: rank r takes r, r+W, r+2W, ..."""
    return list(range(rank, n_items, world_size))


def bce_logits_grad(logits, labels, first_step=0):
    """d/dlogits of the reference loss (pl_module.py:88-120): sum over the classified steps of
    BCEWithLogits(pos_weight = #neg/#pos), mean over edges.  logits [L,E], labels [E] in {0,1}."""
    E = labels.numel()
    pos = labels.sum()
    pw = (E - pos) / pos.clamp(min=1)
    w = torch.where(labels > 0, pw, torch.ones_like(pw))
    g = (torch.sigmoid(logits) * (1 + (pw - 1) * labels) - pw * labels) / max(E, 1)
    if first_step > 0:
        g[:first_step] = 0
    return g, w


def allreduce_mean_(flat, world_size, group=None):
    """In-place all-reduce(sum) / W of a flat gradient bucket (RCCL over xGMI on GPUs, gloo in CPU tests)."""
    if world_size > 1:
        import torch.distributed as dist
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        flat.mul_(1.0 / world_size)
    return flat


class FlatBucket:
    """Parameters AND their gradients as views of two flat fp32 buffers: one collective and one optimizer kernel per
    step.  The parameters' storage is moved into ``flat_params`` (values preserved; ``state_dict`` unaffected)."""

    def __init__(self, params):
        self.params = list(params)
        # every parameter starts on a 16-byte boundary of the flat buffers (padding stays zero: zero gradient, zero update), so
        # that the kernels' 16-byte operand paths apply to the views exactly as to separately allocated tensors
        offs, n = [], 0
        for p in self.params:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4
        dev = self.params[0].device
        # four spare elements behind the gradients: [n] carries a rank's "invalid graph" flag through the all-reduce (TrainStep)
        self.n = n
        self.flat = torch.zeros(n + 4, dtype=torch.float32, device=dev)
        self.flat_params = torch.zeros(n + 4, dtype=torch.float32, device=dev)
        self.views = {}
        self.offsets = dict((id(p), off) for p, off in zip(self.params, offs))
        for p, off in zip(self.params, offs):
            v = self.flat[off:off + p.numel()].view_as(p)
            self.views[id(p)] = v
            pv = self.flat_params[off:off + p.numel()].view_as(p)
            pv.copy_(p.data)
            p.data = pv
            p.grad = v

    def zero_(self):
        self.flat.zero_()


class FlatAdam:
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (the reference's optimizer, pl_module.py:76-77) as ONE
    native kernel over a ``FlatBucket``'s flat parameter / gradient buffers (``mpnhip_adam_step``)."""

    def __init__(self, bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        """``lr`` (like ``betas``, ``eps`` and ``weight_decay``) is read at every ``step()``: assign ``opt.lr`` between two steps to
        follow a learning-rate schedule (all the reference's ``lr_scheduler`` does to the optimizer, pl_module.py:78-86)."""
        self.bucket = bucket
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.exp_avg = torch.zeros_like(bucket.flat_params)
        self.exp_avg_sq = torch.zeros_like(bucket.flat_params)
        self.t = 0   # calls of step()
        # guarded calls that the device-side flag skipped: kept ON the device next to the moments (the host never reads the flag on
        # the ranks whose own graph is fine), so that the bias corrections follow the number of APPLIED updates like torch's Adam
        self.skipped = torch.zeros(4, dtype=torch.int32, device=bucket.flat_params.device)

    @property
    def applied_steps(self):
        """Updates actually applied (a host read of the device-side counter; diagnostics / tests)."""
        return self.t - int(self.skipped[0])

    def step(self, guarded=False):
        """``guarded``: skip the update (on the device, no host read) when the bucket's spare element ``flat[n]`` is non-zero."""
        import ctypes as C
        self.t += 1
        capi._weights_epoch[0] += 1   # raw-pointer update: invalidates packed weight images kept by MOTMPNet.hot_path
        b = self.bucket
        skip = C.c_void_p(b.flat.data_ptr() + 4 * b.n) if guarded else None
        capi.check(capi.load().mpnhip_adam_step_counted(capi.ptr(b.flat_params), capi.ptr(b.flat), capi.ptr(self.exp_avg),
                                                        capi.ptr(self.exp_avg_sq), b.n, C.c_float(self.lr),
                                                        C.c_float(self.betas[0]), C.c_float(self.betas[1]), C.c_float(self.eps),
                                                        C.c_float(self.weight_decay), self.t, skip,
                                                        capi.ptr(self.skipped) if guarded else None, capi.stream_ptr()),
                   "mpnhip_adam_step")


class TrainStep:
    """fwd (saving activations) -> loss gradient -> hand-written bwd into the flat bucket ->
    all-reduce(sum)/W over RCCL (world_size > 1) -> Adam.  Graph prep is cached on `holder`."""

    def __init__(self, model, world_size=1, lr=1e-3, process_group=None, weight_decay=0.0, force_collectives=False,
                 train_mask_branch=False, loss_weights=None):
        """``force_collectives``: issue the step's collectives (and the guarded optimizer step) even at world_size 1 -- a 1-rank
        process group exercises the whole data-parallel code path (RCCL communicator, the side stream as an ExternalStream, two
        asynchronous bucket all-reduces, the join) where only one GPU is available; the result is the single-rank step's.

        ``train_mask_branch``: the joint step of the reference (pl_module.py:88-135) -- tracking BCE and mask BCE optimised together.
        The parameters of ``node_ext_encoder``, ``MPAttentionNet.node_model`` and ``mask_predictor`` (``state_dict`` order) join the
        flat bucket IN FRONT of the hot path's: ``[mask | encoder | message passing + classifier | spare]``.  The encoder's and the
        message-passing segments stay the contiguous ranges ``allreduce_buckets`` reduces, the spare elements (the invalid-graph flag)
        stay at the tail of the collective that is issued last, and one Adam launch covers everything.  The mask branch's convolutions
        and LayerNorm run as stock modules under autograd; its neighbour aggregation and everything else of the step is native.
        ``loss_weights``: ``hparams['train_params']['loss_weights']`` ({'tracking', 'segmentation'}; default 1 and 1)."""
        if not backward_available():
            raise capi.MpnhipError("TrainStep needs mpnhip_backward")
        self.model = model
        self.world_size = world_size
        self.collectives = world_size > 1 or bool(force_collectives)
        self.pg = process_group
        self.train_mask_branch = bool(train_mask_branch)
        lw = dict(loss_weights) if loss_weights is not None else {}
        self.loss_weights = {'tracking': float(lw.get('tracking', 1)), 'segmentation': float(lw.get('segmentation', 1))}
        mask_params = []
        if self.train_mask_branch:
            if not getattr(model, 'has_mask_branch', False):
                raise capi.MpnhipError("train_mask_branch=True needs a model with the mask branch (node_ext_encoder, MPAttentionNet, "
                                       "mask_predictor)")
            if world_size > 1:
                bn = [n for mod in model._mask_modules() for n, m_ in mod.named_modules()
                      if isinstance(m_, torch.nn.modules.batchnorm._BatchNorm)]
                if bn:
                    raise capi.MpnhipError("BatchNorm in the mask branch with world_size %d: every rank would keep running statistics "
                                           "of its own graphs (only the gradients are exchanged)" % world_size)
            mask_params = self.mask_branch_parameters(model)
        # the bucket must not be built before every refusal above: FlatBucket moves the parameters' storage
        self.bucket = FlatBucket(mask_params + list(model.hot_path_parameters()))
        hot = model.hot_path_parameters()
        # flat[:mask_elems]: the mask branch (final first: its gradients come from the autograd pass in front of the native backward).
        # hot_path_parameters(): encoder.node_model, encoder.edge_model, then the message-passing modules and the classifier:
        # flat[mask_elems:enc_elems] is the encoder's bucket (final last, on the caller's stream), flat[enc_elems:] the other one
        self.mask_elems = self.bucket.offsets[id(hot[0])]
        enc = set(id(p) for p in list(model.encoder.node_model.parameters()) + list(model.encoder.edge_model.parameters()))
        first_mp = [p for p in hot if id(p) not in enc][0]
        self.enc_elems = self.bucket.offsets[id(first_mp)]
        self._side = None
        self.opt = FlatAdam(self.bucket, lr=lr, weight_decay=weight_decay)
        self.first_class_step = max(int(model.num_enc_steps) - int(model.num_class_steps), 0)
        self._cmodels = {}
        self._hot_params = hot
        self.last_losses = None

    @staticmethod
    def mask_branch_parameters(model):
        """The mask branch's parameters in ``state_dict`` order."""
        own = set(id(p) for mod in model._mask_modules() for p in mod.parameters())
        return [p for _, p in model.named_parameters() if id(p) in own]

    def native_models(self, n_edges):
        """The native model descriptions (``mpnhip_model``: every weight's and gradient's device address) of the forward and of the
        backward, built once per resolved operand precision and reused: the parameters are views of the bucket's flat buffer and
        the gradients views of its gradient buffer, so the addresses do not change from step to step.  Building one costs 50 - 70 us
        of Python, a step needs several, and at the reference's graph sizes the step is bound by the host (KITTIMOTS-like graph:
        453 us to enqueue a 390 us step, tools/diag/host_cost.py).  The cache is keyed on the parameters' addresses and shapes,
        ``num_enc_steps``, the reattach flags and the aggregation mode."""
        model = self.model
        prec = model.operand_precision(n_edges)
        # everything c_model() bakes into the description besides the precision: the parameters' addresses and shapes (layer
        # dims), the step count, the reattach flags and the aggregation -- a model edited between two steps gets a new description
        agg = getattr(model.MPNet.node_model, "node_agg_fn", None)
        ptrs = (tuple((p.data_ptr(), tuple(p.shape)) for p in self._hot_params), int(model.num_enc_steps),
                bool(model.reattach_initial_nodes), bool(model.reattach_initial_edges), getattr(agg, "code", id(agg)))
        hit = self._cmodels.get(prec)
        if hit is None or hit[0] != ptrs:
            keep_f, keep_b = [], []
            mf = model.c_model(keep_f, n_edges=n_edges)
            mb = model.c_model(keep_b, grads=self.bucket.views, n_edges=n_edges)
            hit = (ptrs, mf, mb, keep_f, keep_b)
            self._cmodels[prec] = hit
        return hit[1], hit[2]

    def allreduce_mask_segment(self):
        """The joint step's first collective: all-reduce(sum) of ``flat[:mask_elems]``, asynchronous, issued as soon as the mask
        branch's autograd pass is enqueued -- those gradients are final there, and the collective runs beside the native backward.
        Returns the work handle ``allreduce_buckets`` waits for (None without a mask segment)."""
        import torch.distributed as dist
        flat, m = self.bucket.flat, self.mask_elems
        if not m:
            return None
        with torch.cuda.device(flat.device):
            return dist.all_reduce(flat[:m], op=dist.ReduceOp.SUM, group=self.pg, async_op=True)

    def allreduce_buckets(self, side_pending, mask_work=None):
        """all-reduce(sum) / W of the flat gradient buffer.  ``side_pending``: the backward left its side stream un-joined
        (MPNHIP_BWD_DEFER_SIDE_JOIN): the message-passing bucket's collective is ordered behind THAT stream, so it overlaps
        the encoder's backward still queued on the caller's stream; the encoder's bucket follows in the caller's order.
        ``mask_work``: the handle of ``allreduce_mask_segment`` (joint step): ``flat[:mask_elems]`` is on its way already and is only
        waited for here; the spare elements travel at the tail of ``flat[enc_elems:]``, the collective issued behind the flag read."""
        import torch.distributed as dist
        flat, k = self.bucket.flat, self.enc_elems
        m = self.mask_elems if mask_work is not None else 0
        with torch.cuda.device(flat.device):
            if side_pending:
                if self._side is None:
                    self._side = torch.cuda.ExternalStream(capi.load().mpnhip_side_stream(), device=flat.device)
                # evidence of the overlap (tests, bench): when the side stream reached the message-passing bucket's collective, and
                # when the caller's stream finished the encoder's backward
                self.ev_mp_ready = torch.cuda.Event(enable_timing=True)
                self.ev_main_done = torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(self._side):
                    self.ev_mp_ready.record()
                    w_mp = dist.all_reduce(flat[k:], op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
                self.ev_main_done.record()
                w_enc = dist.all_reduce(flat[m:k], op=dist.ReduceOp.SUM, group=self.pg, async_op=True) if k > m else None
                w_mp.wait()
                if w_enc is not None:
                    w_enc.wait()
                capi.check(capi.load().mpnhip_side_stream_join(capi.stream_ptr()), "mpnhip_side_stream_join")
            else:
                dist.all_reduce(flat[m:] if m else flat, op=dist.ReduceOp.SUM, group=self.pg)
            if mask_work is not None:
                mask_work.wait()
            flat.mul_(1.0 / self.world_size)

    def _check_joint_inputs(self, x, x_ext, mask_labels, mask_gt_ixs, node_graph, n_graphs):
        """The joint step's refusals, raised BEFORE anything is enqueued: every rank must issue the same collectives."""
        missing = [n for n, t in (("x_ext", x_ext), ("mask_labels", mask_labels), ("mask_gt_ixs", mask_gt_ixs)) if t is None]
        if missing:
            raise capi.MpnhipError("TrainStep(train_mask_branch=True) needs %s" % ", ".join(missing))
        if int(n_graphs) > 1 and node_graph is None:
            raise capi.MpnhipError("a batch of %d graphs needs node_graph for the segmentation loss" % int(n_graphs))
        capi.require_device(x_ext, mask_labels, mask_gt_ixs, node_graph)
        if x_ext.shape[0] != x.shape[0] or mask_labels.shape[0] != x.shape[0]:
            raise capi.MpnhipError("x_ext %s / mask_labels %s do not have x's %d rows"
                                   % (tuple(x_ext.shape), tuple(mask_labels.shape), x.shape[0]))

    def batch(self, b, **kw):
        """One step on a batch dict as ``train_batch.TrainingBatches`` / ``build_batch`` deliver it (``x``, ``edge_index``, ``edge_attr``,
        ``edge_labels``, ``edge_graph``, ``node_graph``, ``n_graphs`` and, for the joint step, ``x_ext``, ``mask_labels``, ``mask_gt_ixs``)."""
        return self(b['x'], b['edge_index'], b['edge_attr'], labels=b.get('edge_labels'), edge_graph=b.get('edge_graph'),
                    n_graphs=int(b.get('n_graphs', 1)), x_ext=b.get('x_ext'), mask_labels=b.get('mask_labels'),
                    mask_gt_ixs=b.get('mask_gt_ixs'), node_graph=b.get('node_graph'), **kw)

    def __call__(self, x, edge_index, edge_attr, labels=None, holder=None, optimizer_step=True, edge_graph=None, n_graphs=1,
                 x_ext=None, mask_labels=None, mask_gt_ixs=None, node_graph=None, log=None):
        """``edge_graph`` / ``n_graphs``: (x, edge_index, edge_attr) is a block-diagonal batch of ``n_graphs`` graphs (int32 graph id per
        edge, ``loss.edge_graph_ids``): ONE forward / backward over the batch with the reference's per-graph loss averaged over the
        graphs -- ``accumulate_grad_batches`` optimizer micro-steps (configs/tracking_cfg.yaml:3-4) executed in space on one GPU.

        ``x_ext`` / ``mask_labels`` / ``mask_gt_ixs`` / ``node_graph`` (joint mode, ``train_mask_branch=True``): the mask branch's
        inputs and targets as ``TrainingBatches`` delivers them.  The native forward's logits become an autograd leaf,
        ``model.mask_predictions`` runs on them under autograd, both loss terms and their gradients come from the native loss
        kernels, ``torch.autograd.backward`` accumulates the mask branch's gradients into their bucket views and the mask loss's
        pull on EVERY step's logits into ``logits.grad``, which joins the tracking gradient in front of the native backward.
        ``log``: an ``EpochLog`` that receives this step's losses and per-graph metric counts (device to device, no host read).
        ``last_loss``: the tracking loss vector [1 + L]; ``last_losses``: {'tracking': [1 + L], 'segmentation': [1 + k]} (device)."""
        from .mpn import _prepared, check_hot_path_inputs
        model = self.model
        joint = self.train_mask_branch
        if joint:
            self._check_joint_inputs(x, x_ext, mask_labels, mask_gt_ixs, node_graph, n_graphs)
            if holder is None:
                holder = _Holder()   # (one graph prep for the hot path and the mask branch's aggregation steps)
        g = _prepared(edge_index, x.shape[0], holder)
        x = capi.f32c(x)
        ea = capi.f32c(edge_attr)
        E = ea.shape[0]
        m_fwd, m_bwd = self.native_models(E)
        check_hot_path_inputs(m_fwd, g, x, ea)
        L = max(int(model.num_enc_steps), 1)
        logits = torch.empty((L, E), dtype=torch.float32, device=x.device)
        ws = native_forward_saved(model, g, x, ea, logits, cmodel=m_fwd)
        if labels is None:
            if getattr(self, "_default_labels", None) is None or self._default_labels.numel() != E:
                self._default_labels = (torch.arange(E, device=x.device) % 7 == 0).float()
            labels = self._default_labels
        # reference loss (pl_module.py:88-107) and its gradient w.r.t. every step's logits, natively
        from .loss import tracking_loss_and_grad
        preds = None
        if joint:
            # the mask branch under autograd on the native forward's logits as a leaf (stock convolutions / LayerNorm, native
            # _AttentionAggregate): its backward below fills the mask parameters' bucket views and logits.grad
            logits.requires_grad_(True)
            with torch.enable_grad():
                preds = model.mask_predictions(x_ext, edge_index, logits, holder=holder)
        self.last_loss, glog = tracking_loss_and_grad(logits.detach() if joint else logits, labels, self.first_class_step,
                                                      self.loss_weights['tracking'], edge_graph=edge_graph, n_graphs=n_graphs)
        self.bucket.zero_()
        mask_work = None
        if joint:
            from .loss import mask_loss_and_grad
            seg_loss, gmask = mask_loss_and_grad(preds, mask_labels, mask_gt_ixs, self.loss_weights['segmentation'],
                                                 node_graph=node_graph, n_graphs=n_graphs)
            self.last_losses = {'tracking': self.last_loss, 'segmentation': seg_loss}
            torch.autograd.backward(preds, grad_tensors=[gm.view_as(p_) for gm, p_ in zip(gmask, preds)])
            if logits.grad is not None:   # the mask loss's pull on every step's logits, the early (unclassified) ones included
                glog += logits.grad
                logits.grad = None
            logits = logits.detach()
            if self.collectives:
                mask_work = self.allreduce_mask_segment()
        else:
            self.last_losses = {'tracking': self.last_loss, 'segmentation': None}
        if log is not None:
            log.append_step(self.last_losses, logits[-1], labels, edge_index, x.shape[0], edge_graph, node_graph, n_graphs, holder)
        lib = capi.load()
        defer = self.collectives and bool(lib.mpnhip_backward_uses_side_stream(m_fwd))
        native_backward(model, g, x, ea, glog, ws, self.bucket.views, defer_side_join=defer, cmodel=m_bwd)
        # IndexError like the reference's x[row] gather for an edge_index outside [0, N) (graph prep clamps such entries and sets a
        # flag): read once per graph, BEFORE anything is done with the gradients of the clamped graph -- the prep finished long
        # before the backward was enqueued, so the read waits for nothing
        err = None
        try:
            g.raise_if_invalid()
        except IndexError as exc:
            err = exc
        if self.collectives:
            # every rank must take part in this step's collectives; the flag rides in a spare element of the bucket, the reduced
            # element guards the optimizer step on every rank (nobody steps on bad gradients), then the offending rank raises
            if err is not None:
                self.bucket.flat[self.bucket.n:].fill_(1.0)
                torch.cuda.current_stream().synchronize()   # (the bucket's collective may run on the library's side stream)
            self.allreduce_buckets(defer, mask_work)
        elif err is not None:
            raise err
        if optimizer_step:
            self.opt.step(guarded=self.collectives)
        if err is not None:
            raise err
        return logits

    @torch.no_grad()
    def evaluate(self, x, edge_index, edge_attr, labels, holder=None, edge_graph=None, n_graphs=1, x_ext=None, mask_labels=None,
                 mask_gt_ixs=None, node_graph=None, log=None):
        """The reference's ``validation_step`` (pl_module.py:122-135 with ``train_val='val'``): forward only, the loss vectors and the
        per-graph metric counts, all left on the device -- ``{'logits': [L, E], 'losses': {'tracking': [1 + L], 'segmentation':
        [1 + k] or None}, 'counts': int32 [n_graphs, 8]}``.  The bucket, the optimizer state and the process group are not touched;
        the mask branch takes the model's ``mask_convs`` route (``'native'``: the native convolutions).  In joint mode the mask
        inputs are required as in the training call.  ``log``: an ``EpochLog`` that receives the result."""
        from .loss import mask_loss_and_grad, step_metric_counts, tracking_loss_and_grad
        model = self.model
        if self.train_mask_branch:
            self._check_joint_inputs(x, x_ext, mask_labels, mask_gt_ixs, node_graph, n_graphs)
        if holder is None:
            holder = _Holder()
        from .mpn import _prepared
        _prepared(edge_index, x.shape[0], holder)   # (the full prep once: the metrics and the attention aggregation need it)
        logits = model.hot_path(capi.f32c(x), edge_index, capi.f32c(edge_attr), holder=holder)
        tl, _ = tracking_loss_and_grad(logits, labels, self.first_class_step, self.loss_weights['tracking'], edge_graph=edge_graph,
                                       n_graphs=n_graphs)
        sl = None
        if self.train_mask_branch:
            preds = model.mask_predictions(x_ext, edge_index, logits, holder=holder)
            sl, _ = mask_loss_and_grad(preds, mask_labels, mask_gt_ixs, self.loss_weights['segmentation'], node_graph=node_graph,
                                       n_graphs=n_graphs)
        losses = {'tracking': tl, 'segmentation': sl}
        out = log.next_counts(n_graphs) if log is not None else None
        counts = step_metric_counts(logits[-1], labels, edge_index, x.shape[0], edge_graph=edge_graph, node_graph=node_graph,
                                    n_graphs=n_graphs, holder=holder, out=out)
        if log is not None:
            log.append(losses, counts, n_graphs)
        return {'logits': logits, 'losses': losses, 'counts': counts}

    # ------------------------------------------------------------------ checkpoint / resume (the reference: ModelCheckpoint)
    def _param_names(self):
        names = dict((id(p), n) for n, p in self.model.named_parameters())
        return [names[id(p)] for p in self.bucket.params]

    def state_dict(self):
        """Everything a resumed run needs, keyed by parameter NAME (not by flat offset, so a checkpoint does not depend on the bucket
        layout): the model's ``state_dict``, Adam's ``exp_avg`` / ``exp_avg_sq`` per parameter, the call count ``t``, the device-side
        count of skipped calls, the optimizer's hyper-parameters, ``train_mask_branch`` and the model's ``mask_conv_grads`` selector
        ('stock', 'native' or 'native_all': which backward the mask branch's convolutions, transposed convolutions and LayerNorm
        took).  Tensors are copies on their device."""
        b, o = self.bucket, self.opt
        names = self._param_names()

        def slices(flat):
            return dict((n, flat[b.offsets[id(p)]:b.offsets[id(p)] + p.numel()].view_as(p).clone()) for n, p in zip(names, b.params))
        return {'model': dict((k, v.detach().clone()) for k, v in self.model.state_dict().items()),
                'exp_avg': slices(o.exp_avg), 'exp_avg_sq': slices(o.exp_avg_sq), 't': int(o.t), 'skipped': o.skipped.clone(),
                'lr': o.lr, 'betas': tuple(o.betas), 'eps': o.eps, 'weight_decay': o.weight_decay,
                'train_mask_branch': self.train_mask_branch, 'mask_conv_grads': getattr(self.model, 'mask_conv_grads', 'stock')}

    def load_state_dict(self, state):
        """Restore ``state_dict()`` into this step (built on a fresh model): weights are written THROUGH the flat views, the moments
        into the flat moment buffers by parameter name.  A hot-path-only checkpoint loads into a joint step (mask moments zero; mask
        weights from the checkpoint's model when it has them), a joint checkpoint into a hot-path-only step (its mask moments are
        ignored).  ``mask_conv_grads`` goes back onto the model.  A hot-path key that is missing or has another shape raises ``MpnhipError`` naming it, before anything is written."""
        b, o = self.bucket, self.opt
        names = self._param_names()
        hot = set(id(p) for p in self._hot_params)
        ck = state['model']
        bad = []
        for n, p in zip(names, b.params):
            if id(p) not in hot:
                continue
            for what, table in (('model', ck), ('exp_avg', state['exp_avg']), ('exp_avg_sq', state['exp_avg_sq'])):
                t = table.get(n)
                if t is None:
                    bad.append("%s[%r] is missing" % (what, n))
                elif tuple(t.shape) != tuple(p.shape):
                    bad.append("%s[%r] is %s, the model's is %s" % (what, n, tuple(t.shape), tuple(p.shape)))
        own = self.model.state_dict()
        for k, v in own.items():
            if k in ck and tuple(ck[k].shape) != tuple(v.shape) and not any(repr(k) in s for s in bad):
                bad.append("model[%r] is %s, the model's is %s" % (k, tuple(ck[k].shape), tuple(v.shape)))
        if bad:
            raise capi.MpnhipError("load_state_dict: " + "; ".join(bad))
        with torch.no_grad():
            for k, v in own.items():     # (state_dict() tensors alias the parameters' storage: the bucket's flat_params)
                if k in ck:
                    v.copy_(ck[k])
            o.exp_avg.zero_()
            o.exp_avg_sq.zero_()
            for n, p in zip(names, b.params):
                off = b.offsets[id(p)]
                for flat, table in ((o.exp_avg, state['exp_avg']), (o.exp_avg_sq, state['exp_avg_sq'])):
                    t = table.get(n)
                    if t is not None and tuple(t.shape) == tuple(p.shape):
                        flat[off:off + p.numel()].view_as(p).copy_(t)
            o.skipped.copy_(state['skipped'])
        o.t = int(state['t'])
        o.lr, o.betas, o.eps, o.weight_decay = state['lr'], tuple(state['betas']), state['eps'], state['weight_decay']
        if 'mask_conv_grads' in state:    # (a checkpoint from before the selector leaves the model's as it is)
            self.model.mask_conv_grads = state['mask_conv_grads']
        capi._weights_epoch[0] += 1   # raw writes into flat_params: packed weight images are stale
        self._cmodels = {}


class _Holder:
    """Owner of one call's cached graph prep (``mpn._prepared``) when the caller passes none."""


class EpochLog:
    """The reference's ``validation_epoch_end`` / training-epoch log (pl_module.py:137-147) without a host read per step: device
    buffers for ``capacity_steps`` steps of up to ``max_graphs`` graphs -- per step the total / tracking / segmentation loss and
    the per-graph counts of ``loss.step_metric_counts``.  ``append`` copies device to device; ``summary()`` is the only host read."""

    def __init__(self, capacity_steps, max_graphs, device=None):
        dev = torch.device(device if device is not None else "cuda")
        self.capacity, self.max_graphs = int(capacity_steps), int(max_graphs)
        if self.capacity < 1 or not 1 <= self.max_graphs <= 1024:
            raise capi.MpnhipError("EpochLog: capacity_steps >= 1 and 1 <= max_graphs <= 1024")
        self.losses = torch.zeros((self.capacity, 2), dtype=torch.float32, device=dev)    # tracking, segmentation
        self.counts = torch.zeros((self.capacity, self.max_graphs, 8), dtype=torch.int32, device=dev)
        self.n_graphs = []   # host: the graphs of every appended step

    def reset(self):
        self.n_graphs = []

    def next_counts(self, n_graphs):
        """The int32 [n_graphs, 8] block of the next step, for ``step_metric_counts(out=...)`` to fill in place."""
        k = int(n_graphs)
        if len(self.n_graphs) >= self.capacity or not 1 <= k <= self.max_graphs:
            raise capi.MpnhipError("EpochLog: step %d of %d with %d graphs (at most %d)" % (len(self.n_graphs) + 1, self.capacity, k,
                                                                                     self.max_graphs))
        return self.counts[len(self.n_graphs), :k]

    def append(self, losses, counts, n_graphs):
        """``losses``: {'tracking': [1 + L], 'segmentation': [1 + k] or None} (device); ``counts``: int32 [n_graphs, 8] (device)."""
        dst = self.next_counts(n_graphs)
        i = len(self.n_graphs)
        if counts.data_ptr() != dst.data_ptr():
            dst.copy_(counts.view(-1, 8))
        self.losses[i, 0:1].copy_(losses['tracking'][0:1])
        if losses.get('segmentation') is not None:
            self.losses[i, 1:2].copy_(losses['segmentation'][0:1])
        else:
            self.losses[i, 1].zero_()
        self.n_graphs.append(int(n_graphs))

    def append_step(self, losses, logits_last, labels, edge_index, num_nodes, edge_graph, node_graph, n_graphs, holder):
        """What ``TrainStep(..., log=self)`` does: the step's counts straight into this log's buffer, then its losses."""
        from .loss import step_metric_counts
        counts = step_metric_counts(logits_last, labels, edge_index, num_nodes, edge_graph=edge_graph, node_graph=node_graph,
                                    n_graphs=n_graphs, holder=holder, out=self.next_counts(n_graphs))
        self.append(losses, counts, n_graphs)

    def summary(self):
        """{'loss', 'loss_tracking', 'loss_segmentation', 'accuracy', 'recall', 'precision', 'constr_sr'}: the mean over ALL graphs of
        the epoch (a step's losses are its graphs' mean: weighted by its ``n_graphs``), NaN entries skipped as
        ``pd.DataFrame(outputs).mean(axis=0)`` skips them (pl_module.py:139-141 with the reference's batch_size 1)."""
        import numpy as np
        from .loss import metrics_from_counts
        s = len(self.n_graphs)
        if s == 0:
            return dict((k, float("nan")) for k in ("loss", "loss_tracking", "loss_segmentation", "accuracy", "recall", "precision",
                                                    "constr_sr"))
        losses = self.losses[:s].cpu().numpy().astype(np.float64)    # (the host read)
        counts = self.counts[:s].cpu().numpy()
        w = np.asarray(self.n_graphs, np.float64)

        def wmean(v):
            ok = ~np.isnan(v)
            return float((v[ok] * w[ok]).sum() / w[ok].sum()) if ok.any() else float("nan")

        def nanmean(v):
            ok = ~np.isnan(v)
            return float(v[ok].mean()) if ok.any() else float("nan")
        out = {"loss": wmean(losses[:, 0] + losses[:, 1]), "loss_tracking": wmean(losses[:, 0]), "loss_segmentation": wmean(losses[:, 1])}
        rows = np.concatenate([counts[i, :k] for i, k in enumerate(self.n_graphs)])
        for k, v in metrics_from_counts(rows).items():
            out[k] = nanmean(v)
        return out
