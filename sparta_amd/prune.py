"""Block pruning for block-sparse layers on VBS handles: a score per stored block (sparta_vbs_block_ssq), a selection rule in torch, and the chosen blocks
written as zeros -- and kept zero through training -- in the weights, the optimizer state and the gradients (sparta_vbs_mask_blocks).  The block pattern
of a handle stays as creation made it: a pruned block is a stored block of zeros, which the fp32 forward product already skips (the k-compaction of
set_values follows the zero pattern of the new values).  A new pattern is a new handle: BlockPruner.compact and .grow move a
layer onto one, with its values and optimizer state (sparta_amd.repattern).  torch is imported when first used, as in optim.py."""
import math


def select(scores, keep, sparsity, scope="global"):
    """The selection rule: which blocks are to be zero at `sparsity`.  Pure torch, any device, no synchronisation.

    scores, keep: lists with one tensor per layer -- a floating-point score per block (low = prune first) and the current mask (uint8 or bool, 0 = pruned).
    Over all blocks (scope "global") or per layer ("layer"): k = floor(sparsity * n_blocks) blocks are to be zero in total.  The blocks already pruned count
    first (they stay pruned: the rule is monotone); then come the live blocks in ascending score order, ties going to the lower (layer, block) index (a
    stable sort).  A non-finite score counts as +Inf: such a block is chosen only when no block with a finite score is left.  With k not above the number
    already pruned nothing changes.  Returns the new masks, a list of uint8 tensors."""
    import torch
    if scope not in ("global", "layer"):
        raise ValueError("scope must be 'global' or 'layer'")
    if not 0.0 <= sparsity <= 1.0:
        raise ValueError("sparsity must lie in [0, 1]")
    if len(scores) != len(keep) or any(s.numel() != k.numel() for s, k in zip(scores, keep)):
        raise ValueError("scores and keep must hold one tensor per layer, of the same lengths")

    def one(s, live):
        n = s.numel()
        k = int(math.floor(sparsity * n))
        s = s.reshape(-1).to(torch.float64)
        inf = torch.full_like(s, float("inf"))
        key = torch.where(live, torch.where(torch.isfinite(s), s, inf), -inf)          # the pruned first, in index order; the non-finite last
        order = torch.sort(key, stable=True).indices
        rank = torch.empty_like(order)
        rank[order] = torch.arange(n, device=order.device)
        return (live & (rank >= k)).to(torch.uint8)

    lives = [k.reshape(-1) != 0 for k in keep]
    if scope == "layer" or len(scores) <= 1:
        return [one(s, l) for s, l in zip(scores, lives)]
    new = one(torch.cat([s.reshape(-1).to(torch.float64) for s in scores]), torch.cat(lives))
    return list(torch.split(new, [k.numel() for k in keep]))


def select_swap(mag_scores, grad_scores, keep, n_swap, scope="global"):
    """The swap rule of dynamic sparse training (RigL, SET): drop the weakest live blocks, grow as many dead ones.  Pure torch, any device, no synchronisation.

    mag_scores, grad_scores, keep: lists with one tensor per layer -- a magnitude score and a gradient score per block, and the current mask (uint8 or bool,
    0 = dead).  Over all layers (scope "global", n_swap an int) or per layer ("layer", n_swap a list with one int per layer):
      drop  the n_swap live blocks with the lowest magnitude score, in select's order: stable, ties to the lower (layer, block) index, a non-finite score last;
      grow  the n_swap blocks with the highest gradient score among those that were dead BEFORE this call (a block dropped now is not grown now): stable,
            ties to the lower index, a non-finite score counts as the lowest, and a block whose score is -inf is never grown (the caller marks the blocks
            without an element inside the matrix that way).
    If either side holds fewer candidates than n_swap both counts shrink to the smaller side, so the number of live blocks never changes; the counts are
    tensors and are compared with the ranks on the device.  Returns the new masks, a list of uint8 tensors."""
    import torch
    if scope not in ("global", "layer"):
        raise ValueError("scope must be 'global' or 'layer'")
    if not (len(mag_scores) == len(grad_scores) == len(keep)) or any(m.numel() != k.numel() or g.numel() != k.numel() for m, g, k in zip(mag_scores, grad_scores, keep)):
        raise ValueError("mag_scores, grad_scores and keep must hold one tensor per layer, of the same lengths")
    per_layer = scope == "layer"
    if per_layer:
        if not isinstance(n_swap, (list, tuple)) or len(n_swap) != len(keep):
            raise ValueError("scope 'layer' takes n_swap as a list with one count per layer")
        counts = [int(n) for n in n_swap]
    else:
        counts = [int(sum(n_swap)) if isinstance(n_swap, (list, tuple)) else int(n_swap)]
    if any(n < 0 for n in counts):
        raise ValueError("n_swap must be >= 0")

    def ranks(key, member):
        """position of every member in ascending key order (stable: ties to the lower index); the others come behind all members"""
        order = torch.sort(key, stable=True).indices
        order = order[torch.sort((~member[order]).to(torch.uint8), stable=True).indices]
        rank = torch.empty_like(order)
        rank[order] = torch.arange(key.numel(), device=order.device)
        return rank

    def one(m, g, live, n):
        m, g = m.reshape(-1).to(torch.float64), g.reshape(-1).to(torch.float64)
        inf = torch.full_like(m, float("inf"))
        cand = ~live & ~(g == -inf)                                                      # (NaN and +Inf may be grown, after every finite score)
        drop_rank = ranks(torch.where(torch.isfinite(m), m, inf), live)
        grow_rank = ranks(torch.where(torch.isfinite(g), -g, inf), cand)
        count = torch.minimum(torch.minimum(live.sum(), cand.sum()), torch.full((), n, dtype=torch.int64, device=m.device))
        return ((live & (drop_rank >= count)) | (cand & (grow_rank < count))).to(torch.uint8)

    lives = [k.reshape(-1) != 0 for k in keep]
    if per_layer:
        return [one(m, g, l, n) for m, g, l, n in zip(mag_scores, grad_scores, lives, counts)]
    if not keep:
        return []
    cat = lambda ts: torch.cat([t.reshape(-1).to(torch.float64) for t in ts])
    new = one(cat(mag_scores), cat(grad_scores), torch.cat(lives), counts[0])
    return list(torch.split(new, [k.numel() for k in keep]))


class BlockProbe:
    """what vbs_linear(probe=...) fills: sel, a uint8 tensor of n_blocks (1 = score this block), and out, a float64 tensor of n_blocks (the scores)"""

    def __init__(self, sel, out):
        self.sel, self.out = sel, out


class BlockPruner:
    """Magnitude pruning of the stored blocks of block-sparse layers, on the device.

        pruner = sa.BlockPruner(opt)              # a VbsSGD / VbsAdamW, or a list of (handle, values) pairs
        ...
        loss.backward(); pruner.mask_grads(); ctl.collect(opt); opt.step(ctl=ctl)          # every step: the gradient of the pruned blocks is zero
        pruner.prune(0.5)                         # now and then: the lowest-scoring blocks of all layers become zero

    The score of a block is the sum of the squares of its values inside the matrix, divided (normalize=True) by their number: block-rows of different heights
    compare, and a ragged last block column is not pruned for being narrow.  scope: "global" ranks the blocks of all pairs together, "layer" each pair alone.
    A pruned block is +0.0 in values, in the optimizer's state and (after mask_grads) in the gradient, and the optimizers' arithmetic keeps it there (W = M =
    V = +0 and g = +-0 give W = +0, with momentum and with either weight decay).  prune, mask_grads and scores are launches and torch device operations only, on
    torch's current stream; mask_grads can be captured into a graph after its first call (the masks are updated in place).

    skip_pruned=True: prune and load_state_dict also hand every handle its mask (DeviceVBS.set_live_blocks), so that the backward products skip the pruned
    blocks instead of computing them: sddmm stores +0.0 for them and spmm_t leaves them out (their values are zero: the same sum).  A gradient that comes from
    vbs_linear alone is then already +0 in the pruned blocks and mask_grads() can be dropped from the loop; it is still needed where anything else adds to
    values.grad (a regulariser, a second use of the values outside vbs_linear).

    live_steps=True (needs skip_pruned=True): the handles are also switched to live steps (DeviceVBS.set_live_steps) once they have their mask, so that the
    optimizer's step skips the pruned blocks too -- it reads and writes the weights, the gradient and the state of the live blocks only, with the bits of the
    plain step.  The pruned blocks of values must stay +0.0, which prune guarantees; their gradient and state are not looked at any more.

    live_forward=True (needs skip_pruned=True): the handles are also switched to the live forward product (DeviceVBS.set_live_forward) once they have their
    mask: the 16-bit forward product of a handle that has the live form walks the steps of the live blocks only.  The values of the pruned blocks are zero,
    so the product is the same, the sign of a zero aside; handles without the live form (fp32 among them) keep their kernels.

    a8_live=True (needs skip_pruned=True, excludes live_forward=True): for handles whose fp8 weight image is on (DeviceVBS.set_forward_a8) -- the handles are
    switched to the live form of the product on that image (DeviceVBS.set_a8_live) once they have their mask.  A handle with the fp8 switch off raises there.

    Regrowing (dynamic sparse training): pass probe(i) to pair i's vbs_linear(..., probe=...) and backward leaves the squared gradient norm of every PRUNED
    block in it (DeviceVBS.sddmm_block_ssq: the live sddmm no longer computes those gradients).  regrow(fraction) then swaps: the weakest live blocks are
    pruned and as many pruned blocks with the largest gradient come back, as zeros -- the number of live blocks stays what prune made it.

    Changing the pattern: compact(vbmats) drops the pruned blocks for good -- every pair moves onto a fresh handle that stores its live blocks only, with its
    values and the optimizer's state (sparta_amd.repattern) -- and grow(i, vbmat, add) adds blocks the pattern does not store.  Both replace handles, values,
    masks and probes by new objects of the new sizes: fetch pairs, keep_masks() and probe(i) again afterwards."""

    def __init__(self, optimizer_or_pairs, scope="global", normalize=True, skip_pruned=False, live_steps=False, live_forward=False, a8_live=False):
        import torch
        if scope not in ("global", "layer"):
            raise ValueError("scope must be 'global' or 'layer'")
        if live_steps and not skip_pruned:
            raise ValueError("live_steps=True needs skip_pruned=True (the steps skip the blocks of the live set the handles are given)")
        if live_forward and not skip_pruned:
            raise ValueError("live_forward=True needs skip_pruned=True (the forward product skips the blocks of the live set the handles are given)")
        if a8_live and not skip_pruned:
            raise ValueError("a8_live=True needs skip_pruned=True (the product on the fp8 image skips the blocks of the live set the handles are given)")
        if a8_live and live_forward:
            raise ValueError("a8_live=True and live_forward=True exclude each other (live forward is refused while the fp8 weight image is on)")
        self.live_forward = bool(live_forward)
        self.a8_live = bool(a8_live)
        self.optimizer = optimizer_or_pairs if hasattr(optimizer_or_pairs, "pairs") else None
        self.pairs = [(h, v) for h, v in (self.optimizer.pairs if self.optimizer is not None else optimizer_or_pairs)]
        self.scope, self.normalize, self.skip_pruned, self.live_steps = scope, bool(normalize), bool(skip_pruned), bool(live_steps)
        self._keep, self._n_in, self._probes = [], [], []
        for handle, values in self.pairs:
            self._keep.append(torch.ones(handle.n_blocks, dtype=torch.uint8, device=values.device))
            self._n_in.append(handle.block_ssq(torch.ones_like(values, requires_grad=False)))          # 1 + 1 + ...: the elements inside the matrix, exactly
            self._probes.append(BlockProbe(torch.zeros(handle.n_blocks, dtype=torch.uint8, device=values.device),
                                           torch.zeros(handle.n_blocks, dtype=torch.float64, device=values.device)))
        sizes = [k.numel() for k in self._keep]
        self._live = sizes if self._per_layer() else [sum(sizes)]   # live blocks per pair, kept on the host; scope "global" knows only their sum

    def scores(self):
        """per pair: block_ssq(values), divided by the block's elements inside the matrix when normalize (a block without any scores +Inf)"""
        import torch
        out = []
        for (handle, values), n_in in zip(self.pairs, self._n_in):
            s = handle.block_ssq(values.detach())
            if self.normalize:
                s = torch.where(n_in > 0, s / n_in, torch.full_like(s, float("inf")))
            out.append(s)
        return out

    def _state_tensors(self, i):
        opt = self.optimizer
        if opt is None:
            return []
        if hasattr(opt, "_bufs"):
            return [opt._bufs[i]] if opt._bufs[i] is not None else []
        s = opt._state[i] if hasattr(opt, "_state") else None
        return [] if s is None else [s["exp_avg"], s["exp_avg_sq"]]

    def _apply(self, i):
        handle, values = self.pairs[i]
        tensors = [values.detach()] + ([values.grad] if values.grad is not None else []) + self._state_tensors(i)
        handle.mask_blocks(self._keep[i], *tensors)
        self._probes[i].sel.copy_(self._keep[i] == 0)
        handle.set_values(values.detach())
        if self.skip_pruned:
            handle.set_live_blocks(self._keep[i])
            if self.live_steps:
                handle.set_live_steps(True)
            if self.live_forward:
                handle.set_live_forward(True)
            if self.a8_live:
                handle.set_a8_live(True)

    def prune(self, sparsity):
        """select() on scores(), then per pair the pruned blocks zeroed in values, values.grad (if present) and the optimizer's state (where allocated), and
        the handle given the new values"""
        new = select(self.scores(), self._keep, sparsity, self.scope)
        for i, k in enumerate(new):
            self._keep[i].copy_(k)
            self._apply(i)
        # select is exact by count: floor(sparsity * blocks) are pruned per scope, or as many as were already
        sizes = [k.numel() for k in self._keep]
        if self._per_layer():
            self._live = [min(l, n - int(math.floor(sparsity * n))) for l, n in zip(self._live, sizes)]
        else:
            self._live = [min(sum(self._live), sum(sizes) - int(math.floor(sparsity * sum(sizes))))]

    def _per_layer(self):
        return self.scope == "layer" or len(self.pairs) <= 1

    def probe(self, i):
        """pair i's probe for vbs_linear(..., probe=...): .sel (uint8, n_blocks) is kept equal to keep == 0 in place by prune, regrow and load_state_dict,
        .out (float64, n_blocks) takes the scores of the pruned blocks in backward.  compact and grow replace the probe of a pair they move: fetch it again"""
        return self._probes[i]

    def regrow(self, fraction):
        """One swap of dynamic sparse training.  Per scope n_swap = floor(fraction * live blocks) (counted on the host: prune is exact by count and a swap
        keeps the count); select_swap on scores() and the probes' .out -- divided by the block's elements inside the matrix when normalize, -inf for a
        block without any -- updates the masks in place.  Then per pair what prune does: the dropped blocks become +0.0 in values, values.grad and the
        optimizer's state (the grown ones are +0.0 everywhere already: that is what prune maintains), the handle gets the values, its live set and the live
        switches, and the probe's .sel follows.  Launches and torch device operations only.  The probes must hold the scores of a backward that ran with
        the current masks."""
        import torch
        if not 0.0 <= fraction <= 1.0:
            raise ValueError("fraction must lie in [0, 1]")
        grad = []
        for p, n_in in zip(self._probes, self._n_in):
            g = p.out / n_in if self.normalize else p.out
            grad.append(torch.where(n_in > 0, g, torch.full_like(g, float("-inf"))))
        if self._per_layer():
            new = select_swap(self.scores(), grad, self._keep, [int(math.floor(fraction * l)) for l in self._live], "layer")
        else:
            new = select_swap(self.scores(), grad, self._keep, int(math.floor(fraction * self._live[0])), "global")
        for i, k in enumerate(new):
            self._keep[i].copy_(k)
            self._apply(i)

    def _prepare_pair(self, i, vbmat, keep, add, block_row_range):
        """the first half of pair i's repattern (sparta_amd.repattern_prepare), through the optimizer where there is one: may refuse, changes nothing"""
        if self.optimizer is not None:
            return self.optimizer.repattern_prepare(i, vbmat, keep=keep, add=add, block_row_range=block_row_range)
        from .device import repattern_prepare
        return repattern_prepare(vbmat, self.pairs[i][0], [self.pairs[i][1].detach()], keep=keep, add=add, block_row_range=block_row_range)

    def _commit_pair(self, i, plan):
        """the second half: pair i on its new pattern (the optimizer's state travels); returns (new_vbmat, map)"""
        if self.optimizer is not None:
            new_vbmat, handle, values = self.optimizer.repattern_commit(i, plan)
            bmap = self.optimizer.last_map
        else:
            from .device import repattern_commit
            old = self.pairs[i][1]
            new_vbmat, handle, new_t, bmap = repattern_commit(plan)
            values = new_t[0].requires_grad_(old.requires_grad)
        self.pairs[i] = (handle, values)
        return new_vbmat, bmap

    def compact(self, vbmats, block_row_ranges=None):
        """The pruned blocks dropped for good: every pair moves onto the pattern of its live blocks (VbsSGD / VbsAdamW.repattern(i, vbmat, keep=mask), or
        sparta_amd.repattern on values where the pruner was given pairs), so that the handle's images, values and the optimizer's state hold the live blocks
        only and the planner deals the steps anew.  vbmats: per pair the VBR its handle was created from; block_row_ranges: per pair the range its handle was
        created with (None: whole matrices).  Afterwards the pruner starts afresh on the new sizes: all-ones masks, new block sizes, zeroed probes, every
        block live -- keep_masks() and probe(i) return NEW tensors, and pairs / optimizer.pairs hold new handles and new leaf values (grad None): fetch
        them again.  The new handles carry no live set (they have no dead blocks); the next prune installs one.  The old handles stay open.  Synchronises.
        Every pair is prepared (sparta_amd.repattern_prepare: the new handle, and whether it qualifies for the fp8 weight image the old one multiplies with)
        before any pair is moved: a refusal closes the new handles, raises, and leaves pruner and optimizer as they were -- all pairs compact, or none.
        Returns the new vbmats."""
        import torch
        if len(vbmats) != len(self.pairs):
            raise ValueError("compact needs one vbmat per pair")
        plans = []
        try:
            for i, vbmat in enumerate(vbmats):
                br = None if block_row_ranges is None else block_row_ranges[i]
                plans.append(self._prepare_pair(i, vbmat, self._keep[i], None, br))
        except Exception:
            for plan in plans:
                plan.close()
            raise
        out = []
        for i, plan in enumerate(plans):
            try:
                new_vbmat, _ = self._commit_pair(i, plan)
            except Exception:
                for later in plans[i + 1:]:
                    later.close()
                raise
            out.append(new_vbmat)
            handle, values = self.pairs[i]
            self._keep[i] = torch.ones(handle.n_blocks, dtype=torch.uint8, device=values.device)
            self._n_in[i] = handle.block_ssq(torch.ones_like(values, requires_grad=False))
            self._probes[i] = BlockProbe(torch.zeros(handle.n_blocks, dtype=torch.uint8, device=values.device),
                                         torch.zeros(handle.n_blocks, dtype=torch.float64, device=values.device))
        sizes = [k.numel() for k in self._keep]
        self._live = sizes if self._per_layer() else [sum(sizes)]
        return out

    def grow(self, i, vbmat, add, block_row_range=None):
        """Pair i grown beyond its stored pattern: the blocks of `add` -- (block-row, block column) pairs the pattern does not store -- are added, as zeros in
        values and in the optimizer's state, and are LIVE.  The masks, the block sizes and the probe are re-laid through the block map: existing blocks keep
        their entries (a pruned block stays pruned and stored), added ones get keep = 1 and a probe score of 0.  With skip_pruned=True the new handle gets the
        live set and the pruner's live switches again.  keep_masks()[i] and probe(i) are NEW tensors, and the pair holds a new handle and new leaf values.
        To choose the blocks, score candidates the handle does not store with a pattern-only handle of the candidates and sddmm_block_ssq.
        Synchronises.  Returns the new vbmat."""
        import torch
        add = [(int(a), int(b)) for a, b in add]
        old_keep, old_out = self._keep[i], self._probes[i].out
        new_vbmat, bmap = self._commit_pair(i, self._prepare_pair(i, vbmat, None, add, block_row_range))      # (a refusal raises before anything is replaced)
        handle, values = self.pairs[i]
        m = torch.from_numpy(bmap.astype("int64")).to(values.device)
        old = m >= 0
        src = m.clamp(min=0)
        keep = torch.ones(handle.n_blocks, dtype=torch.uint8, device=values.device)
        keep[old] = old_keep[src[old]]
        out = torch.zeros(handle.n_blocks, dtype=torch.float64, device=values.device)
        out[old] = old_out[src[old]]
        self._keep[i] = keep
        self._n_in[i] = handle.block_ssq(torch.ones_like(values, requires_grad=False))
        self._probes[i] = BlockProbe((keep == 0).to(torch.uint8), out)
        self._live[i if self._per_layer() else 0] += len(add)
        if self.skip_pruned:
            handle.set_live_blocks(keep)
            if self.live_steps:
                handle.set_live_steps(True)
            if self.live_forward:
                handle.set_live_forward(True)
            if self.a8_live:
                handle.set_a8_live(True)
        return new_vbmat

    def mask_grads(self):
        """the gradient of every pruned block made zero: call it after backward and before GradCtl.collect / step, so that the clipped norm is that of the
        live blocks and the step leaves the pruned ones at zero"""
        for (handle, values), keep in zip(self.pairs, self._keep):
            if values.grad is not None:
                handle.mask_blocks(keep, values.grad)

    def keep_masks(self):
        """per pair the mask, a uint8 device tensor of n_blocks elements (0 = pruned); updated in place by prune.  compact and grow change the number of blocks:
        after them this returns NEW tensors, of the new sizes"""
        return list(self._keep)

    def sparsity(self):
        """pruned blocks / blocks over all pairs (synchronises)"""
        total = sum(k.numel() for k in self._keep)
        pruned = sum(int((k == 0).sum().item()) for k in self._keep)
        return pruned / total if total else 0.0

    def state_dict(self):
        """{"keep": [per pair the mask as a uint8 CPU tensor], "scope", "normalize"} (synchronises)"""
        return {"keep": [k.detach().cpu().clone() for k in self._keep], "scope": self.scope, "normalize": self.normalize}

    def load_state_dict(self, sd):
        """takes the masks over and applies them as prune does: values, gradient and optimizer state of the pruned blocks become zero, the handles get the
        new values"""
        import torch
        if len(sd["keep"]) != len(self.pairs):
            raise ValueError("the state dict holds %d pairs, the pruner %d" % (len(sd["keep"]), len(self.pairs)))
        for i, src in enumerate(sd["keep"]):
            if src.numel() != self._keep[i].numel():
                raise ValueError("pair %d: the mask holds %d blocks, expected %d" % (i, src.numel(), self._keep[i].numel()))
        self.scope, self.normalize = sd.get("scope", self.scope), bool(sd.get("normalize", self.normalize))
        for i, src in enumerate(sd["keep"]):
            self._keep[i].copy_((src != 0).to(torch.uint8))
            self._apply(i)
        live = [int((src != 0).sum().item()) for src in sd["keep"]]                    # (synchronises if the masks are device tensors)
        self._live = live if self._per_layer() else [sum(live)]
