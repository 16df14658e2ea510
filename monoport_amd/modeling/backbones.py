"""Image encoders of the PIFu networks, run once per frame.  On an MI355X (eval mode, fp32, 512 x 512
and up) both run as chains of hand-written kernels only (``_forward_dataflow``, csrc/conv3x3.hip /
convim2col.hip / encoder_ops.hip / gn_tail.h); anything else -- CPU tensors, training, odd shapes,
``MONOPORT_ENCODER_DATAFLOW=off`` -- takes the per-module paths below (MIOpen convolutions and / or
round 2's fused kernels).

Only the two encoders the reference's configs select are provided:

* ``HGFilter`` / ``PIFuHGFilters``      -- 4-stack hourglass, netG  (backbones/HGFilters.py:117-216)
* ``ResnetFilter`` / ``PIFuResBlkFilters`` -- 6 residual blocks, netC (backbones/ResBlkFilters.py:87-147)

Parameter names and shapes follow the reference's state dicts exactly, so ``load_state_dict`` /
``load_legacy_pifu`` accept the published checkpoints.  The modules are written for inference:
the forward passes avoid in-place aliasing tricks and keep activations in whatever memory format
the caller chose (``.to(memory_format=torch.channels_last)`` is honoured end to end).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

import contextlib
import os
import threading

_GROUPS = 32  # GroupNorm(32, C) everywhere (HGFilters.py:23-27, ResBlkFilters.py:19)
# "hip" (default): the pyramid blocks' GroupNorm -> ReLU -> conv3x3 chains run as the fused f32-MFMA
# kernels of csrc/conv3x3.hip; "miopen": stock convolutions + the stand-alone GroupNorm kernel
ENCODER_CONV = os.environ.get("MONOPORT_ENCODER_CONV", "hip")
# ... on feature maps of at least this height (all of the hourglass's maps: with 32-pixel tiles the
# kernels match or beat MIOpen's convolution alone down to 32x32 and save its GroupNorm pass,
# tools/conv_probe.py / profiles/r02m_conv_probe.txt)
ENCODER_CONV_MIN_H = 32
# arithmetic of those kernels: "f32" (exact f32 MFMA) or "f16x3" (f32 emulated on f16 MFMA: every
# operand split into two halves, three MFMAs per product term, f32 accumulation -- the encoder-side
# counterpart of SurfaceClassifier.set_precision("f16x3"))
ENCODER_CONV_PRECISION = os.environ.get("MONOPORT_ENCODER_CONV_PRECISION", "f32")
# "on" (default): the whole encoder runs as a chain of hand-written kernels with every GroupNorm handed
# from the kernel that writes a tensor to the kernel that reads it (csrc/gn_tail.h); "off": round 2's
# per-module fused kernels with stand-alone statistics / finalize launches and the MIOpen stem
ENCODER_DATAFLOW = os.environ.get("MONOPORT_ENCODER_DATAFLOW", "on")


def set_encoder_conv_precision(precision):
    """Process-wide switch for the fused 3x3 convolutions ("f32" / "f16x3"); takes effect on the
    next forward (captured hipGraphs must be re-captured: FrameSlot.prepare())."""
    global ENCODER_CONV_PRECISION
    if precision not in ("f32", "f16x3"):
        raise ValueError("encoder conv precision must be 'f32' or 'f16x3'")
    ENCODER_CONV_PRECISION = precision


_repeatable_lock = threading.Lock()
_repeatable_state = [0, False]  # passes inside, the flag as the first one found it


@contextlib.contextmanager
def _repeatable_convs(x, module):
    """While an inference pass on the GPU is inside, torch's own convolutions (the per-module paths: sizes the HIP
    kernels do not take, MONOPORT_ENCODER_CONV=miopen) pick among MIOpen's deterministic solvers only.  Its default
    choice for Conv2d(128, 64, 3, padding=1) on a 48 x 40 map -- HGFilter on a 384 x 320 image -- gave another
    rounding of the same sums on 9 of 10 calls (7e-7 there, 1e-5 at the encoder's output), while every kernel of
    csrc/ is bit-repeatable.  The flag is torch's process-wide one, so passes in several threads share it: the first
    one in sets it, the last one out puts back what the first found."""
    if not x.is_cuda or module.training or not _inference_only(x, module):
        yield
        return
    st = _repeatable_state
    with _repeatable_lock:
        if st[0] == 0:
            st[1] = torch.backends.cudnn.deterministic
            torch.backends.cudnn.deterministic = True
        st[0] += 1
    try:
        yield
    finally:
        with _repeatable_lock:
            st[0] -= 1
            if st[0] == 0:
                torch.backends.cudnn.deterministic = st[1]


class _GroupNorm(nn.GroupNorm):
    """nn.GroupNorm (same parameters / state-dict keys) whose inference forward on the GPU is the
    split-reduction HIP kernel of csrc/encoder_ops.hip, optionally fused with the ReLU that
    follows every norm but one in these encoders.  CPU tensors, training mode and unusual shapes
    take the stock PyTorch op."""

    def forward(self, x, relu=False):
        if not self.training and ops.group_norm_supported(x) and _inference_only(x, self):
            return ops.group_norm(x, self.num_groups, self.weight, self.bias, self.eps, relu)
        y = super().forward(x)
        return F.relu(y) if relu else y


class _GNReLU(nn.Module):
    """ReLU placeholder used inside nn.Sequential right after a _GroupNorm: the pair is executed
    as one fused call by _run_sequential."""

    def forward(self, x):
        return F.relu(x)


def _gn(channels):
    return _GroupNorm(_GROUPS, channels)


def _run_sequential(seq, x):
    """nn.Sequential forward that fuses each (_GroupNorm, ReLU) pair."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, _GroupNorm) and i + 1 < len(mods) and isinstance(mods[i + 1], (nn.ReLU, _GNReLU)):
            x = m(x, relu=True)
            i += 2
        else:
            x = m(x)
            i += 1
    return x


def _upsample2x_add(low, skip):
    """skip + bicubic x2 (align_corners=True) of ``low`` (HGFilters.py:108-111)."""
    if low.is_cuda and low.dtype == torch.float32 and _inference_only(low, skip):
        return ops.upsample_bicubic2x(low.contiguous(), add=skip.contiguous())
    return skip + F.interpolate(low, scale_factor=2, mode="bicubic", align_corners=True)


def _packed_conv(owner, conv):
    """conv's weight in MFMA fragment order (cached on ``owner``), re-packed when the parameter
    or the encoder precision changes."""
    cache = owner.__dict__.setdefault("_packed_cache", {})
    w = conv.weight
    key = (w.data_ptr(), w._version, str(w.device), ENCODER_CONV_PRECISION)
    hit = cache.get(id(conv))
    if hit is None or hit[0] != key:
        hit = (key, ops.PackedConv3x3(w, ENCODER_CONV_PRECISION))
        cache[id(conv)] = hit
    return hit[1]


def _inference_only(*tensors_or_modules):
    """The ctypes kernels return tensors without a grad_fn: take them only when nothing asks for
    gradients (eval mode with autograd on -- saliency, fine-tuning with frozen statistics -- keeps the
    differentiable PyTorch ops, as the reference modules would)."""
    if not torch.is_grad_enabled():
        return True
    for t in tensors_or_modules:
        if isinstance(t, nn.Module):
            if any(p.requires_grad for p in t.parameters()):
                return False
        elif t is not None and t.requires_grad:
            return False
    return True


def _pow2(v):
    return v > 0 and (v & (v - 1)) == 0


# "on": a drop-in call of an encoder (netG.filter(image) from a stage thread, RTL/main.py:366-370) replays
# its ~135 launches as ONE hipGraph captured on first use per (shape, flags); outputs are copied out of
# the graph's buffers, so they are ordinary tensors that outlive the call (RTL/dataloader.py:1048-1054).
# Default "off": measured on the MI355X box the chain is GPU-bound even launch by launch (batch 1: 4.03
# ms eager, 3.99 ms replayed; single-frame latency 10.6 vs 10.9 ms with the extra copies), so the graph
# only pays on a host too loaded to issue 135 C-ABI calls in 4 ms.  Batches above
# ENCODER_GRAPH_MAX_BATCH always run eagerly (FramePipeline captures its own graph of the whole slot).
ENCODER_GRAPH = os.environ.get("MONOPORT_ENCODER_GRAPH", "off")
# "on" (default): at small batches (latency mode: a drop-in netG.filter(image) call) the skip branch of
# every hourglass level runs on a side stream next to the low-resolution chain; larger batches and
# hipGraph captures stay on one stream (the chip is full, and parallel graph branches measured slower)
# A drop-in encoder call at batch <= ENCODER_PLAN_MAX_BATCH can record its launches once per (shape, flags,
# stream) into an mp_plan (csrc/plan.hip: the same C-ABI calls with the same argument structs, side streams and
# joins included) and replay them with ONE foreign call per frame: 0.7-1.0 ms of host time instead of 2.5-3.4 ms,
# and the interpreter re-acquires its global lock once instead of 137 times.  Outputs are copied out of the plan's
# static buffers (ordinary tensors that outlive the call, RTL/dataloader.py:1048-1054).  Measured (round 5,
# tools/enc_plan_probe.py, profiles/r05d_encoder_plan.txt): the GPU is no faster for it -- 3.2-3.4 ms per call back
# to back either way, and a lone call even 0.1-0.4 ms SLOWER (with every launch queued at once the skip branch's
# large convolutions compete with the long chain of small ones on the critical path) -- so it pays exactly where the
# host is the bottleneck: in a per-frame stage thread of a StagePipeline, next to seven other threads that want the
# interpreter (118-125 -> 130-133 recon/s).  A coalescing stage wants the opposite (its batches form while the
# stage is busy: 158 -> 146 with plans), and a caller that runs the stages one after the other in one thread has
# no contention to remove.  Hence the default "auto": plans only in per-frame StagePipeline stage threads;
# "on": every call at the batch bound; "off": never.
ENCODER_PLAN = os.environ.get("MONOPORT_ENCODER_PLAN", "auto")
ENCODER_PLAN_MAX_BATCH = int(os.environ.get("MONOPORT_ENCODER_PLAN_MAX_BATCH", "2"))
# "on" (default): stacks 0-2 hand over to the next stack with ONE folded 1x1 GEMM over y = relu(bn_end(conv_last(.)))
# instead of [bl | al] over (y, l(y)) (HGFilter._tail_packed), and with last_only -- the stacks' own outputs are
# not asked for -- their l GEMM is skipped altogether; "off": always the reference's three GEMMs
ENCODER_FOLD_TAIL = os.environ.get("MONOPORT_ENCODER_FOLD_TAIL", "on")
ENCODER_BRANCHES = os.environ.get("MONOPORT_ENCODER_BRANCHES", "on")
ENCODER_BRANCH_MAX_BATCH = int(os.environ.get("MONOPORT_ENCODER_BRANCH_MAX_BATCH", "2"))
ENCODER_GRAPH_MAX_BATCH = int(os.environ.get("MONOPORT_ENCODER_GRAPH_MAX_BATCH", "4"))


class _GraphedForward:
    """Per-module cache of captured forwards: key -> (graph, static input, static outputs)."""

    MAX_ENTRIES = 20

    def __init__(self):
        self.entries = {}
        self.lock = threading.Lock()

    @staticmethod
    def fingerprint(module):
        """Cheap identity of the parameters a captured graph baked in (packed copies keyed on data
        pointer / version): changes after load_state_dict, .to(), in-place updates."""
        ver = 0
        first = last = None
        for p in module.parameters():
            ver += p._version
            if first is None:
                first = p
            last = p
        return (ver, first.data_ptr() if first is not None else 0, last.data_ptr() if last is not None else 0)

    def run(self, key, x, fn):
        """fn(x_static) -> flat tuple of tensors / None.  Returns fresh copies of the outputs."""
        with self.lock:
            entry = self.entries.get(key)
            if entry is None:
                cur = torch.cuda.current_stream(x.device)
                side = torch.cuda.Stream(device=x.device)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    x_static = x.clone()
                    fn(x_static)  # eager warm-up: weight packs, scratch arenas
                    side.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                        outs = fn(x_static)
                    side.synchronize()
                # a coalescing stage (stage_pipeline.Coalesced) meets every batch size from 1 to its max_batch:
                # keep that many captures, and when shapes keep changing beyond that drop the one that has not
                # been used for the longest time (clearing all of them re-captured ~1.7 s per shape, over and over)
                while len(self.entries) >= self.MAX_ENTRIES:
                    self.entries.pop(next(iter(self.entries)))
                entry = self.entries[key] = (graph, x_static, outs)
            else:
                self.entries[key] = self.entries.pop(key)  # most recently used last
            graph, x_static, outs = entry
            x_static.copy_(x)
            graph.replay()
            return tuple(None if o is None else o.clone() for o in outs)


# "on" (default): the pass a plan is recorded from allocates out of a PRIVATE allocator pool (torch.cuda.MemPool)
# and keeps no reference to its intermediates, so the caching allocator recycles blocks inside the pass exactly
# as it does launch by launch (~200 MB per image instead of ~1 GB of separately-held intermediates) and nobody
# else is ever handed those blocks.  "off": every intermediate stays alive on its own.  Speed is the same either
# way (measured: single-frame latency 8.15 / 8.19 ms): the pool is about memory, not about cache locality.
ENCODER_PLAN_POOL = os.environ.get("MONOPORT_ENCODER_PLAN_POOL", "on")


class _PlannedForward:
    """Per-module cache of recorded forwards: key -> (plan, static input, static outputs)."""

    MAX_ENTRIES = 6  # (shape, flags, stream) combinations kept

    def __init__(self):
        self.entries = {}
        self.lock = threading.Lock()

    @staticmethod
    def _record(x, fn):
        # The private pool is only private if torch routes THIS THREAD's allocations into it: torch >= 2.7
        # (torch._C._cuda_beginAllocateCurrentThreadToPool; the installed 2.10 has it).  Older versions route
        # every thread's allocations on the device into the pool while the context is open, so a neighbouring
        # stage thread's tensor could land in a block the plan later overwrites on replay: keep the
        # intermediates alive there instead (keep_alive=True, no recycling to get wrong).
        use_pool = (ENCODER_PLAN_POOL == "on" and hasattr(torch.cuda, "MemPool")
                    and hasattr(torch._C, "_cuda_beginAllocateCurrentThreadToPool"))
        if not use_pool:
            x_static = x.clone()
            with ops.record_plan(x.device, keep_alive=True) as rec:
                outs = fn(x_static)
            return rec.finish(), x_static, outs, None
        fn(x)  # launch by launch once, OUTSIDE the pool: weight packs, scratch arenas, side streams
        pool = torch.cuda.MemPool()
        with torch.cuda.use_mem_pool(pool, device=x.device):
            x_static = x.clone()
            # Recycling inside the pass is safe under replay: a block is handed out again on the stream it was
            # allocated on, behind its last use in that stream's order; a use on another stream is followed by
            # a join (ops.plan_wait) before the owner stream runs on -- and a replay keeps both orders.
            with ops.record_plan(x.device, keep_alive=False) as rec:
                outs = fn(x_static)
        return rec.finish(), x_static, outs, pool

    def run(self, key, x, fn):
        """fn(x_static) -> flat tuple of tensors / None.  Returns fresh copies of the outputs."""
        with self.lock:
            entry = self.entries.get(key)
            if entry is None:
                plan, x_static, outs, pool = self._record(x, fn)  # a real pass: its results are this call's results
                while len(self.entries) >= self.MAX_ENTRIES:
                    self.entries.pop(next(iter(self.entries)))
                self.entries[key] = (plan, x_static, outs, pool)
            else:
                self.entries[key] = self.entries.pop(key)  # most recently used last
                plan, x_static, outs, _ = entry
                x_static.copy_(x)
                plan.run(x.device)
            return tuple(None if o is None else o.clone() for o in outs)


def _plan_wanted(x):
    if ENCODER_PLAN == "auto":
        from ..stage_pipeline import stage_kind
        if stage_kind() != "stage":
            return False
    elif ENCODER_PLAN != "on":
        return False
    return (x.shape[0] <= ENCODER_PLAN_MAX_BATCH and not torch.cuda.is_current_stream_capturing()
            and ops._recording() is None)


def _graph_wanted(x, graphed):
    if graphed is None:
        graphed = ENCODER_GRAPH == "on" and x.shape[0] <= ENCODER_GRAPH_MAX_BATCH
    return bool(graphed) and not torch.cuda.is_current_stream_capturing()


def _block_dataflow(blk, x, acc_x, arena, out_stats=False):
    """ConvBlock (HGFilters.py:40-62) as three launches of csrc/conv3x3.hip (+ one 1x1 launch for a
    projection shortcut) and nothing else: every GroupNorm is handed from the kernel that writes a
    tensor to the kernel that reads it (``acc_x``: the accumulator x's producer filled; bn1 and bn4
    read the same statistics with their own affine parameters), and torch.cat((out1, out2, out3), 1)
    + residual is written by the three epilogues.  ``out_stats``: also collect the statistics of the
    block's output.  Returns (out, accumulator of out or None)."""
    n, c_in, h, w = x.shape
    ca, cb, cc = blk.conv1.out_channels, blk.conv2.out_channels, blk.conv3.out_channels
    if blk.downsample is None:
        shortcut = x
    else:
        shortcut = ops.conv1x1_fused(x, (acc_x, blk.bn4), True, None, blk._packed_projection())
    out = torch.empty((n, ca + cb + cc, h, w), dtype=torch.float32, device=x.device)
    acc_out = arena.take() if out_stats else None
    acc_a, acc_b = arena.take(), arena.take()
    a = ops.conv3x3_fused(x, (acc_x, blk.bn1), blk._packed(blk.conv1), stats=acc_a, out=out, res=shortcut,
                          out_off=0, out_stats=acc_out)
    b = ops.conv3x3_fused(a, (acc_a, blk.bn2), blk._packed(blk.conv2), stats=acc_b, out=out, res=shortcut,
                          out_off=ca, out_stats=acc_out)
    ops.conv3x3_fused(b, (acc_b, blk.bn3), blk._packed(blk.conv3), want_y=False, out=out, res=shortcut,
                      out_off=ca + cb, out_stats=acc_out)
    return out, acc_out


class ConvBlock(nn.Module):
    """Pre-activation pyramid block: three GN-ReLU-3x3 convs of widths C/2, C/4, C/4 whose
    outputs are concatenated and added to a (projected) shortcut (HGFilters.py:12-62)."""

    def __init__(self, c_in, c_out):
        super().__init__()
        half, quarter = c_out // 2, c_out // 4
        self.conv1 = nn.Conv2d(c_in, half, 3, 1, 1, bias=False)
        self.conv2 = nn.Conv2d(half, quarter, 3, 1, 1, bias=False)
        self.conv3 = nn.Conv2d(quarter, quarter, 3, 1, 1, bias=False)
        self.bn1 = _gn(c_in)
        self.bn2 = _gn(half)
        self.bn3 = _gn(quarter)
        self.bn4 = _gn(c_in)  # always present in the checkpoints, used only by the projection
        if c_in != c_out:
            # indices 0 / 2 carry parameters: "downsample.0.*" aliases bn4, "downsample.2.weight"
            self.downsample = nn.Sequential(self.bn4, nn.ReLU(), nn.Conv2d(c_in, c_out, 1, bias=False))
        else:
            self.downsample = None

    def _packed(self, conv):
        return _packed_conv(self, conv)

    def _fused_ok(self, x):
        if self.training or ENCODER_CONV != "hip" or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            return False
        if not _inference_only(x, self):
            return False
        h, w = x.shape[2], x.shape[3]
        min_h = ENCODER_CONV_MIN_H if ENCODER_CONV_PRECISION == "f32" else min(ENCODER_CONV_MIN_H, 32)
        # conv1 and conv2 also emit the statistics bn2 / bn3 read: widths whose groups straddle the kernels'
        # channel blocks (Cout = 96, 192 ... of a ConvBlock(., 384)) stay on the torch ops
        return (h >= min_h and (h * w) % 4 == 0 and all(ops.conv3x3_supported(c.in_channels, c.out_channels, h, w)
                                         for c in (self.conv1, self.conv2, self.conv3))
                and all(ops.conv3x3_stats_supported(c.out_channels) for c in (self.conv1, self.conv2)))

    def _forward_fused(self, x):
        """GroupNorm -> ReLU -> conv3x3, three times, as three kernels: the normalisation is
        applied while the input tile is staged, each convolution's epilogue leaves the partial
        sums the next GroupNorm needs (csrc/conv3x3.hip); only bn1 needs a statistics pass of
        its own (its input comes from another block)."""
        x = x.contiguous()
        n, c_in, h, w = x.shape
        hw = h * w
        stats_x = ops.gn_stats(x, _GROUPS)
        ss = ops.gn_finalize(stats_x, n, c_in, _GROUPS, (c_in // _GROUPS) * hw,
                             self.bn1.weight, self.bn1.bias, self.bn1.eps)
        a, st = ops.conv3x3_gn(x, ss, self._packed(self.conv1), relu=True, want_stats=True)
        ca = a.shape[1]
        ss = ops.gn_finalize(st, n, ca, _GROUPS, (ca // _GROUPS) * hw, self.bn2.weight, self.bn2.bias,
                             self.bn2.eps)
        b, st = ops.conv3x3_gn(a, ss, self._packed(self.conv2), relu=True, want_stats=True)
        cb = b.shape[1]
        ss = ops.gn_finalize(st, n, cb, _GROUPS, (cb // _GROUPS) * hw, self.bn3.weight, self.bn3.bias,
                             self.bn3.eps)
        c, _ = ops.conv3x3_gn(b, ss, self._packed(self.conv3), relu=True, want_stats=False)
        if self.downsample is None:
            shortcut = x
        elif c_in % 64 == 0 and hw % 64 == 0 and self.downsample[2].out_channels in (128, 256):
            # relu(bn4(x)) from the statistics bn1 already took (same input, other affine) applied
            # while the 1x1 projection stages its input (csrc/conv3x3.hip conv1x1_kernel)
            ss4 = ops.gn_finalize(stats_x, n, c_in, _GROUPS, (c_in // _GROUPS) * hw,
                                  self.bn4.weight, self.bn4.bias, self.bn4.eps)
            shortcut, _ = ops.conv1x1(x, ss4, True, None, self._packed_projection())
        else:
            shortcut = _run_sequential(self.downsample, x)
        return ops.concat3_add(a, b, c, shortcut)

    def _packed_projection(self):
        cache = self.__dict__.setdefault("_packed_cache", {})
        w = self.downsample[2].weight
        key = (w.data_ptr(), w._version, str(w.device), ENCODER_CONV_PRECISION)
        hit = cache.get("projection")
        if hit is None or hit[0] != key:
            hit = (key, ops.PackedConv1x1(w, None, precision=ENCODER_CONV_PRECISION))
            cache["projection"] = hit
        return hit[1]

    def forward(self, x):
        if self._fused_ok(x):
            return self._forward_fused(x)
        a = self.conv1(self.bn1(x, relu=True))
        b = self.conv2(self.bn2(a, relu=True))
        c = self.conv3(self.bn3(b, relu=True))
        shortcut = x if self.downsample is None else _run_sequential(self.downsample, x)
        if not self.training and ops.concat3_add_supported(a, b, c, shortcut) and _inference_only(a, b, c, shortcut):
            return ops.concat3_add(a, b, c, shortcut)  # one pass instead of cat + add
        return torch.cat((a, b, c), 1) + shortcut


class HourGlass(nn.Module):
    """Recursive hourglass of ``depth`` levels; children are named b1_k / b2_k / b3_k (+ b2_plus_1
    at the bottom) as in HGFilters.py:75-86."""

    def __init__(self, depth, channels):
        super().__init__()
        self.depth = depth
        for level in range(depth, 0, -1):
            self.add_module("b1_%d" % level, ConvBlock(channels, channels))
            self.add_module("b2_%d" % level, ConvBlock(channels, channels))
        self.add_module("b2_plus_1", ConvBlock(channels, channels))
        for level in range(1, depth + 1):
            self.add_module("b3_%d" % level, ConvBlock(channels, channels))

    def _level(self, level, x):
        skip = getattr(self, "b1_%d" % level)(x)
        y = getattr(self, "b2_%d" % level)(F.avg_pool2d(x, 2, stride=2))
        y = self._level(level - 1, y) if level > 1 else self.b2_plus_1(y)
        y = getattr(self, "b3_%d" % level)(y)
        # bicubic x2, align_corners=True, plus the skip (HGFilters.py:108-111) in one kernel
        return _upsample2x_add(y, skip)

    def forward(self, x):
        return self._level(self.depth, x)

    def first_norm(self):
        """The GroupNorm that reads the hourglass input first (b1 of the outermost level)."""
        return getattr(self, "b1_%d" % self.depth).bn1

    def _level_dataflow(self, level, x, acc_x, arena, sides=None):
        """_level on the hand-over kernels: ``acc_x`` = statistics of x from x's producer (read by
        b1_level.bn1); the returned tensor comes with the statistics its reader needs (b3 of the
        enclosing level, or top_m).  Same evaluation order as HGFilters.py:87-111.
        ``sides``: one side stream per level -- the skip branch b1(x) (three convolutions on the large
        map) then runs next to the low-resolution chain, whose ~20 small launches leave most of the
        chip idle at batch 1; joined before the upsample-add (latency mode, see HGFilter)."""
        b1, b2, b3 = (getattr(self, "b%d_%d" % (k, level)) for k in (1, 2, 3))
        side = sides[level - 1] if sides else None
        if side is None:
            skip, _ = _block_dataflow(b1, x, acc_x, arena)
            y, acc_u = self._low_chain(level, x, arena, sides)
        else:
            # skip branch first (three launches, enqueued at once) on the side stream, then the long
            # low-resolution chain on the caller's stream.  The other way round -- chain on a
            # high-priority side stream, skip filling in -- measured no gain (3.97 vs 3.84 ms at batch
            # 1): the host needs ~1 ms to enqueue the chain before the skip branch would even start
            cur = torch.cuda.current_stream(x.device)
            ops.plan_wait(side, cur)  # side.wait_stream(cur): x and its statistics are complete on cur's timeline
            with torch.cuda.stream(side):
                skip, _ = _block_dataflow(b1, x, acc_x, arena)
            x.record_stream(side)
            y, acc_u = self._low_chain(level, x, arena, sides)
            ops.plan_wait(cur, side)
            skip.record_stream(cur)
        return ops.upsample_add_gn(y, skip, acc_u), acc_u

    def _low_chain(self, level, x, arena, sides):
        """avg-pool -> b2 -> (inner level | b2_plus_1) -> b3 of one hourglass level; returns the tensor
        to upsample and the accumulator the upsample-add will fill."""
        b2, b3 = getattr(self, "b2_%d" % level), getattr(self, "b3_%d" % level)
        acc_p = arena.take()
        pooled = ops.avgpool2_gn(x, acc_p)
        y, acc_y = _block_dataflow(b2, pooled, acc_p, arena, out_stats=True)
        if level > 1:
            y, acc_y = self._level_dataflow(level - 1, y, acc_y, arena, sides)
        else:
            y, acc_y = _block_dataflow(self.b2_plus_1, y, acc_y, arena, out_stats=True)
        y, _ = _block_dataflow(b3, y, acc_y, arena)
        return y, arena.take()


class HGFilter(nn.Module):
    """Stacked-hourglass encoder: [B,3,512,512] -> num_stack x ([B,256,128,128],)
    (HGFilters.py:117-204 with the PIFu settings of :207-216: group norm, ave_pool down)."""

    def __init__(self, num_stack=4, depth=2, dim=256):
        super().__init__()
        self.num_stack = num_stack
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3)
        self.bn1 = _gn(64)
        self.conv2 = ConvBlock(64, 128)
        self.conv3 = ConvBlock(128, 128)
        self.conv4 = ConvBlock(128, 256)
        for i in range(num_stack):
            self.add_module("m%d" % i, HourGlass(depth, 256))
            self.add_module("top_m_%d" % i, ConvBlock(256, 256))
            self.add_module("conv_last%d" % i, nn.Conv2d(256, 256, 1))
            self.add_module("bn_end%d" % i, _gn(256))
            self.add_module("l%d" % i, nn.Conv2d(256, dim, 1))
            if i < num_stack - 1:
                self.add_module("bl%d" % i, nn.Conv2d(256, 256, 1))
                self.add_module("al%d" % i, nn.Conv2d(dim, 256, 1))

    def _tail_packed(self, i):
        """Fragment-order weights of stack i's 1x1 convolutions: conv_last, l and [bl | al]."""
        cache = self.__dict__.setdefault("_tail_cache", {})
        mods = [getattr(self, "conv_last%d" % i), getattr(self, "l%d" % i)]
        if i < self.num_stack - 1:
            mods += [getattr(self, "bl%d" % i), getattr(self, "al%d" % i)]
        key = tuple((p.data_ptr(), p._version) for m in mods for p in (m.weight, m.bias)) + (ENCODER_CONV_PRECISION,)
        hit = cache.get(i)
        if hit is None or hit[0] != key:
            pr = ENCODER_CONV_PRECISION
            packs = [ops.PackedConv1x1(mods[0].weight, mods[0].bias, precision=pr),
                     ops.PackedConv1x1(mods[1].weight, mods[1].bias, precision=pr)]
            if len(mods) == 4:
                packs.append(ops.PackedConv1x1(mods[2].weight, mods[2].bias, mods[3].weight, mods[3].bias,
                                               precision=pr))
                # bl and l read the SAME tensor y = relu(bn_end(conv_last(.))) (HGFilters.py:187-204), so when a
                # stack's own output l(y) is not asked for (last_only: MonoPortNet.query keeps feats_stages[-1]
                # only, MonoPortNet.py:63-64) the stack's hand-over  x + bl(y) + al(l(y))  is ONE 256 x 256 GEMM:
                #     x + (W_bl + W_al W_l) y + (b_bl + W_al b_l + b_al)
                # -- the l GEMM and half of the [bl | al] GEMM (4.3 of a stack's 8.6 GFLOP of 1x1 work) are gone.
                # Folded in float64, rounded once; the result differs from the two-GEMM form by f32 rounding only
                # (another association of the same sums: tests/test_encoder_dataflow_gpu.py::test_folded_tail_*).
                w_l, b_l = mods[1].weight.detach().double().flatten(1), mods[1].bias.detach().double()
                w_bl, b_bl = mods[2].weight.detach().double().flatten(1), mods[2].bias.detach().double()
                w_al, b_al = mods[3].weight.detach().double().flatten(1), mods[3].bias.detach().double()
                w_f = (w_bl + w_al @ w_l).float().contiguous()
                b_f = (b_bl + w_al @ b_l + b_al).float().contiguous()
                packs.append(ops.PackedConv1x1(w_f, b_f, precision=pr))
            hit = (key, packs)
            cache[i] = hit
        return hit[1]

    def _tail_fused(self, i, y, x, hwc_out, want_nchw):
        """conv_last -> bn_end -> ReLU -> l, and x + bl(.) + al(.), as three fused GEMMs
        (csrc/conv3x3.hip: conv1x1_kernel): bn_end's statistics come out of conv_last's epilogue,
        its normalisation + ReLU are applied while l / [bl | al] stage their input, biases and the
        residual are added in the epilogues, and the last stack's features can be written straight
        into the channels-last map the query kernels read (HGFilters.py:184-204)."""
        packs = self._tail_packed(i)
        bn = getattr(self, "bn_end%d" % i)
        n, _, h, w = y.shape
        t, st = ops.conv1x1(y, None, False, None, packs[0], want_stats=True)
        ss = ops.gn_finalize(st, n, 256, _GROUPS, 8 * h * w, bn.weight, bn.bias, bn.eps)
        last = i == self.num_stack - 1
        out, _ = ops.conv1x1(t, ss, True, None, packs[1], want_nchw=want_nchw or not last,
                             y_hwc=hwc_out if last else None)
        if not last:
            x, _ = ops.conv1x1(t, ss, True, out, packs[2], res=x)
        return out, x

    def _dataflow_ok(self, x):
        """The whole encoder on the hand-over kernels: inference, f32 images whose maps are powers of
        two down to 32 x 32 at the bottom of the hourglass (512 x 512 and up)."""
        if self.training or ENCODER_CONV != "hip" or ENCODER_DATAFLOW != "on" or not x.is_cuda:
            return False
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not _inference_only(x, self):
            return False
        h, w = x.shape[2], x.shape[3]
        depth = self.m0.depth
        return (_pow2(h) and _pow2(w) and (h >> (2 + depth)) >= 8 and (w >> (2 + depth)) >= 32
                and ops.convk_supported(3, 64, 7, 2, h, w))

    def _stem_packed(self):
        cache = self.__dict__.setdefault("_tail_cache", {})
        w, b = self.conv1.weight, self.conv1.bias
        key = (w.data_ptr(), w._version, b.data_ptr(), b._version)
        hit = cache.get("stem")
        if hit is None or hit[0] != key:
            hit = (key, ops.PackedConvK(w, b))
            cache["stem"] = hit
        return hit[1]

    def _forward_dataflow(self, x, last_only, hwc_out, keep_nchw):
        """HGFilters.py:167-204 as a chain of hand-written kernels only (no MIOpen / torch op but the
        one fill that clears the GroupNorm accumulators): stem 7x7 (csrc/convim2col.hip) -> GroupNorm +
        ReLU -> pyramid blocks / hourglasses / 1x1 tails, every GroupNorm handed from producer to
        consumer (csrc/gn_tail.h)."""
        depth = self.m0.depth
        blocks = 3 + self.num_stack * (3 * depth + 2)
        arena = ops.GnArena(x.device, x.shape[0], 3 * blocks + self.num_stack * (2 * depth + 2) + 8)
        sides = None
        if (ENCODER_BRANCHES == "on" and x.shape[0] <= ENCODER_BRANCH_MAX_BATCH
                and not torch.cuda.is_current_stream_capturing()):
            cache = self.__dict__.setdefault("_side_streams", {})
            sides = cache.get(str(x.device))
            if sides is None:
                sides = cache[str(x.device)] = [torch.cuda.Stream(device=x.device) for _ in range(depth)]
            arena.buf.record_stream(sides[0])
            for st in sides[1:]:
                arena.buf.record_stream(st)
        c2, c3, c4 = self.conv2, self.conv3, self.conv4
        acc = arena.take()
        t = ops.convk(x, None, False, self._stem_packed(), 2, stats=acc)
        acc_x = arena.take()
        x = ops.gn_apply(t, (acc, self.bn1), True, stats=acc_x)
        y, _ = _block_dataflow(c2, x, acc_x, arena)
        acc = arena.take()
        y = ops.avgpool2_gn(y, acc)
        y, acc = _block_dataflow(c3, y, acc, arena, out_stats=True)
        x, acc_x = _block_dataflow(c4, y, acc, arena, out_stats=True)
        outputs = []
        for i in range(self.num_stack):
            hg, top = getattr(self, "m%d" % i), getattr(self, "top_m_%d" % i)
            last = i == self.num_stack - 1
            y, acc_y = hg._level_dataflow(hg.depth, x, acc_x, arena, sides)
            y, _ = _block_dataflow(top, y, acc_y, arena)
            packs = self._tail_packed(i)
            acc_t = arena.take()
            t = ops.conv1x1_fused(y, None, False, None, packs[0], stats=acc_t)
            bn_end = (acc_t, getattr(self, "bn_end%d" % i))
            fold = not last and ENCODER_FOLD_TAIL == "on"
            if fold and last_only:  # nobody reads this stack's l(y)
                outputs.append((None,))
            else:
                want_nchw = not last or keep_nchw or not (last_only and hwc_out is not None)
                out = ops.conv1x1_fused(t, bn_end, True, None, packs[1], want_nchw=want_nchw,
                                        y_hwc=hwc_out if last else None)
                outputs.append((out,))
            if not last:
                acc_x = arena.take()
                if fold:  # x + bl(y) + al(l(y)) as ONE folded GEMM over y (_tail_packed)
                    x = ops.conv1x1_fused(t, bn_end, True, None, packs[3], res=x, stats=acc_x)
                else:
                    x = ops.conv1x1_fused(t, bn_end, True, out, packs[2], res=x, stats=acc_x)
        return outputs[-1:] if last_only else outputs

    def forward(self, x, last_only=False, hwc_out=None, keep_nchw=False, graphed=None):
        """``last_only=True`` skips materialising the per-stack outputs nobody reads in eval mode
        (MonoPortNet.py:63-64 keeps feats_stages[-1] only); the default matches the reference.
        ``hwc_out`` ([B,H,W,256], fused path only): the LAST stack's features are written there in
        channels-last layout by the producing kernel (no NCHW -> HWC pass); with ``last_only`` the
        NCHW copy is then skipped and the returned entry is None, unless ``keep_nchw``.
        ``graphed``: replay the kernel chain as one hipGraph (None = the ENCODER_GRAPH policy)."""
        if self._dataflow_ok(x):
            x = x.contiguous()
            planned = graphed is None and _plan_wanted(x) and not _graph_wanted(x, None)
            if not planned and not _graph_wanted(x, graphed):
                return self._forward_dataflow(x, last_only, hwc_out, keep_nchw)
            cache = (self.__dict__.setdefault("_plans", _PlannedForward()) if planned
                     else self.__dict__.setdefault("_graphs", _GraphedForward()))
            key = (tuple(x.shape), str(x.device), bool(last_only), hwc_out is not None, bool(keep_nchw),
                   ENCODER_CONV_PRECISION, _GraphedForward.fingerprint(self))
            if planned:  # a plan's buffers are static: one plan per stream that replays it, and per branch policy
                key += (torch.cuda.current_stream(x.device).cuda_stream, ENCODER_BRANCHES, ENCODER_BRANCH_MAX_BATCH)

            def run(xs):
                hwc = torch.empty((xs.shape[0], xs.shape[2] // 4, xs.shape[3] // 4, 256), dtype=torch.float32,
                                  device=xs.device) if hwc_out is not None else None
                outs = self._forward_dataflow(xs, last_only, hwc, keep_nchw)
                return tuple(o[0] for o in outs) + (hwc,)

            flat = cache.run(key, x, run)
            if hwc_out is not None:
                hwc_out.copy_(flat[-1].reshape(hwc_out.shape))
            return [(o,) for o in flat[:-1]]
        with _repeatable_convs(x, self):  # torch's convolutions: the stem, and whatever the kernels do not take
            x = self.bn1(self.conv1(x), relu=True)
            x = F.avg_pool2d(self.conv2(x), 2, stride=2)
            x = self.conv4(self.conv3(x))
            fused = (not self.training and ENCODER_CONV == "hip" and ops.conv1x1_supported(x)
                     and x.shape[1] == 256)
            pack_after = hwc_out is not None and not fused  # no producing kernel to write it: pack the NCHW result
            outputs = []
            for i in range(self.num_stack):
                y = getattr(self, "top_m_%d" % i)(getattr(self, "m%d" % i)(x))
                if fused:
                    nchw = keep_nchw or pack_after or not (last_only and hwc_out is not None)
                    out, x = self._tail_fused(i, y, x, None if pack_after else hwc_out, want_nchw=nchw)
                    outputs.append((out,))
                    continue
                y = getattr(self, "bn_end%d" % i)(getattr(self, "conv_last%d" % i)(y), relu=True)
                out = getattr(self, "l%d" % i)(y)
                outputs.append((out,))
                if i < self.num_stack - 1:
                    x = x + getattr(self, "bl%d" % i)(y) + getattr(self, "al%d" % i)(out)
            if pack_after:  # train mode / MONOPORT_ENCODER_CONV=miopen / odd shapes: same contract, one more pass
                last = outputs[-1][0]
                for b in range(last.shape[0]):
                    ops.pack_features(last[b:b + 1].detach(), out=hwc_out[b])
            return outputs[-1:] if last_only else outputs


    def plan_count(self):
        """Recorded mp_plans (one per shape / flags / stream that replays it, at most _PlannedForward.MAX_ENTRIES)
        plus captured hipGraphs this encoder holds right now -- each owns ~200 MB of static buffers; the soak leg
        of bench.py asserts the count stays flat."""
        d = self.__dict__
        return (len(d["_plans"].entries) if "_plans" in d else 0) + (len(d["_graphs"].entries) if "_graphs" in d else 0)


def PIFuHGFilters(*args, **kwargs):
    return HGFilter(num_stack=4, depth=2, dim=256)


class _ResBlock(nn.Module):
    """x + conv_block(x) with reflect padding (ResBlkFilters.py:28-84); children sit in a
    Sequential named conv_block so that checkpoint keys line up (indices 1, 2, 5, 6)."""

    def __init__(self, dim, last=False):
        super().__init__()
        layers = [nn.ReflectionPad2d(1), nn.Conv2d(dim, dim, 3, bias=False), _gn(dim), nn.ReLU(),
                  nn.ReflectionPad2d(1), nn.Conv2d(dim, dim, 3, bias=False)]
        if not last:
            layers.append(_gn(dim))
        self.conv_block = nn.Sequential(*layers)

    def _fused_ok(self, x):
        if self.training or ENCODER_CONV != "hip" or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            return False
        if not _inference_only(x, self):
            return False
        c = self.conv_block[1]
        return ((x.shape[2] * x.shape[3]) % 4 == 0 and ops.conv3x3_supported(c.in_channels, c.out_channels,
                                                                            x.shape[2], x.shape[3])
                and ops.conv3x3_stats_supported(c.out_channels))  # the GroupNorms read the convolutions' statistics

    def _forward_fused(self, x):
        """Two kernels + the residual: the reflection padding is index arithmetic in the staging
        loop of csrc/conv3x3.hip, the first GroupNorm + ReLU is applied while the second
        convolution stages its input, the last GroupNorm (no ReLU) is folded into the add."""
        x = x.contiguous()
        n, c, h, w = x.shape
        blk = self.conv_block
        t, st = ops.conv3x3_gn(x, None, _packed_conv(self, blk[1]), relu=False, want_stats=True, reflect=True)
        ss = ops.gn_finalize(st, n, c, _GROUPS, (c // _GROUPS) * h * w, blk[2].weight, blk[2].bias, blk[2].eps)
        last = len(blk) == 6
        u, st = ops.conv3x3_gn(t, ss, _packed_conv(self, blk[5]), relu=True, want_stats=not last, reflect=True)
        if last:
            return x + u
        ss = ops.gn_finalize(st, n, c, _GROUPS, (c // _GROUPS) * h * w, blk[6].weight, blk[6].bias, blk[6].eps)
        return ops.scale_shift_add(u, ss, x)

    def _forward_dataflow(self, x, arena):
        """_forward_fused with the GroupNorms handed from kernel to kernel (no statistics / finalize
        launches): two reflect-padded convolutions + the x + GroupNorm(.) tail."""
        blk = self.conv_block
        last = len(blk) == 6
        acc_t = arena.take()
        t = ops.conv3x3_fused(x, None, _packed_conv(self, blk[1]), relu=False, reflect=True, stats=acc_t)
        acc_u = None if last else arena.take()
        u = ops.conv3x3_fused(t, (acc_t, blk[2]), _packed_conv(self, blk[5]), relu=True, reflect=True, stats=acc_u)
        return x + u if last else ops.gn_apply(u, (acc_u, blk[6]), False, res=x)

    def forward(self, x):
        if self._fused_ok(x):
            return self._forward_fused(x)
        return x + _run_sequential(self.conv_block, x)


class ResnetFilter(nn.Module):
    """netC encoder: reflect-pad 7x7, two stride-2 convs, six residual blocks ->
    [([B,256,128,128],)] (ResBlkFilters.py:87-139 with group norm, no tanh: :142-147)."""

    def __init__(self, input_nc=3, ngf=64, n_blocks=6):
        super().__init__()
        layers = [nn.ReflectionPad2d(3), nn.Conv2d(input_nc, ngf, 7, bias=False), _gn(ngf), nn.ReLU()]
        ch = ngf
        for _ in range(2):
            layers += [nn.Conv2d(ch, 2 * ch, 3, 2, 1, bias=False), _gn(2 * ch), nn.ReLU()]
            ch *= 2
        for i in range(n_blocks):
            layers.append(_ResBlock(ch, last=(i == n_blocks - 1)))
        self.model = nn.Sequential(*layers)

    def _dataflow_ok(self, x):
        if self.training or ENCODER_CONV != "hip" or ENCODER_DATAFLOW != "on" or not x.is_cuda:
            return False
        if x.dtype != torch.float32 or x.dim() != 4 or not _inference_only(x, self):
            return False
        m = self.model
        if not (len(m) >= 11 and isinstance(m[1], nn.Conv2d) and m[1].kernel_size == (7, 7)
                and m[1].in_channels == 3 and m[1].bias is None):
            return False
        h, w = x.shape[2], x.shape[3]
        return (_pow2(h) and _pow2(w) and h >= 32 and w >= 256
                and ops.convk_supported(3, m[1].out_channels, 7, 1, h, w)
                and ops.convk_supported(m[4].in_channels, m[4].out_channels, 3, 2, h, w)
                and ops.convk_supported(m[7].in_channels, m[7].out_channels, 3, 2, h // 2, w // 2)
                # every convolution of the chain hands its statistics to the next GroupNorm
                and all(ops.conv3x3_stats_supported(c.out_channels) for c in (m[1], m[4], m[7])))

    def _packed_k(self, conv):
        cache = self.__dict__.setdefault("_packed_cache", {})
        w = conv.weight
        key = (w.data_ptr(), w._version, str(w.device))
        hit = cache.get(id(conv))
        if hit is None or hit[0] != key:
            hit = (key, ops.PackedConvK(w, conv.bias))
            cache[id(conv)] = hit
        return hit[1]

    def _forward_dataflow(self, x):
        """ResBlkFilters.py:111-139 on hand-written kernels only: reflect-padded 7x7 and the two
        stride-2 convolutions on csrc/convim2col.hip (each applies the previous GroupNorm + ReLU while
        it gathers its input and hands its own statistics on), then the residual blocks."""
        m = self.model
        blocks = list(m)[10:]
        arena = ops.GnArena(x.device, x.shape[0], 3 + 2 * len(blocks))
        a0, a1, a2 = arena.take(), arena.take(), arena.take()
        t = ops.convk(x, None, False, self._packed_k(m[1]), 1, reflect=True, stats=a0)
        t = ops.convk(t, (a0, m[2]), True, self._packed_k(m[4]), 2, stats=a1)
        t = ops.convk(t, (a1, m[5]), True, self._packed_k(m[7]), 2, stats=a2)
        x = ops.gn_apply(t, (a2, m[8]), True)
        for blk in blocks:
            x = blk._forward_dataflow(x, arena)
        return [(x,)]

    def forward(self, x, graphed=None):
        if self._dataflow_ok(x):
            x = x.contiguous()
            if not _graph_wanted(x, graphed):
                return self._forward_dataflow(x)
            cache = self.__dict__.setdefault("_graphs", _GraphedForward())
            key = (tuple(x.shape), str(x.device), ENCODER_CONV_PRECISION, _GraphedForward.fingerprint(self))
            return [cache.run(key, x, lambda xs: (self._forward_dataflow(xs)[0][0],))]
        with _repeatable_convs(x, self):
            return [(_run_sequential(self.model, x),)]


def PIFuResBlkFilters(*args, **kwargs):
    return ResnetFilter()
