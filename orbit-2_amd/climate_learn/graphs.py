"""hipGraph capture of the launch-bound part of a training step.

The small configurations (interm_8m / interm_117m on 32 x 64 grids) issue ~1000 kernels of a few microseconds per step:
the GPU waits for the Python launch loop.  `GraphedTrainStep` records zero_grad + forward + loss + (scaled) backward once
into a hipGraph (`torch.cuda.CUDAGraph`) and replays it with a single launch; the optimizer / loss-scaler step stays
eager (its arguments -- learning rate, bias corrections, found_inf handling -- change every step).

Dropout / DropPath seeds are kernel ARGUMENTS, frozen at capture.  The captured sequence therefore begins with
`orbit2_seed_salt(odd constant, add)`: a one-thread kernel that advances a device-side salt every seeded kernel xors into
its seed, so each replay draws new masks while forward and backward of one replay still agree.

With several ranks (or ORBIT2_FORCE_COLLECTIVES=1) the engine's bucket all-reduces are issued during the captured
backward on the communication stream; the body ends with `finish_grad_sync()`, which joins that stream back into the
capture, so the collectives and their overlap with the rest of backward become part of the graph (RCCL supports stream
capture).  Every rank must capture and replay in lock-step, as with any collective."""
from typing import Optional

import torch

from . import _hip
from .trainer import training_step

SALT_STEP = 0x9E3779B97F4A7C15       # odd: the salt walks through all 2^64 values

# Capture mode.  Under the runtime's default ("global") ANY thread of the process that makes a capture-unsafe HIP call while a
# capture is open invalidates the capture -- and the call itself fails.  A process that has an RCCL process group has such a
# thread: ProcessGroupNCCL's watchdog polls hipEventQuery on the end events of every collective it still tracks (the warm-up
# passes' bucket all-reduces); when its query lands inside a global-mode capture it gets hipErrorStreamCaptureUnsupported, throws
# from a non-Python thread, and the process ends in std::terminate -> SIGABRT (round 4's driver run; DESIGN 2, "GPU suite hygiene").  Whether it lands
# there is a race against its 100 ms poll.  "thread_local" restricts the check to the capturing thread.  That is safe for this
# body because everything the capture must not see is already excluded by construction: every kernel of the step is launched
# from THIS thread on the capturing stream or on the engine's communication stream forked from it by an event recorded inside
# the capture; no other thread of ours launches work, allocates or synchronises (the data loader threads only touch host memory
# and pinned buffers); the allocator's own hipMalloc inside a capture is already wrapped in a relaxed-mode guard by PyTorch;
# and the watchdog's event queries concern streams' PAST work, which a capture does not reorder.
CAPTURE_ERROR_MODE = "thread_local"


def _quiesce_collectives(device):
    """Host-synchronises the device and gives the process-group watchdog time to retire every collective it tracks, so that no
    event of an uncaptured collective is still being polled when the capture opens (belt to CAPTURE_ERROR_MODE's braces: with the
    work list empty the watchdog makes no HIP call at all)."""
    import time
    import torch.distributed as dist
    torch.cuda.synchronize(device)
    if dist.is_available() and dist.is_initialized() and dist.get_backend() != "gloo":
        time.sleep(0.35)                             # > 3 watchdog polls (kWatchdogThreadSleepMillis = 100)
        torch.cuda.synchronize(device)


# The seed salt is ONE word per device (include/orbit2_hip.h: orbit2_seed_salt): two engines replaying captured steps on one
# device would advance each other's masks -- each replay still agrees with itself (forward and backward of a replay read the
# same salt), but "the n-th replay of engine A draws mask n" no longer holds, and an eager step of A between two replays of B
# sees B's salt.  The restriction was only documented; it is asserted here: a second LIVE engine with a captured
# step on the same device is refused unless ORBIT2_ALLOW_SHARED_SALT=1 says the caller accepts interleaved mask sequences.
_GRAPHED_ENGINES = {}        # device index -> weakref to the engine that owns the device's salt


def _claim_salt(engine, device):
    import os
    import weakref
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ref = _GRAPHED_ENGINES.get(idx)
    cur = ref() if ref is not None else None
    if cur is not None and cur is not engine and os.environ.get("ORBIT2_ALLOW_SHARED_SALT", "0") != "1":
        raise RuntimeError("GraphedTrainStep: another engine already replays a captured step on cuda:%d and the dropout seed salt "
                           "is one word per device (orbit2_seed_salt): their mask sequences would interleave.  Drop the other "
                           "engine, or set ORBIT2_ALLOW_SHARED_SALT=1 to accept that" % idx)
    _GRAPHED_ENGINES[idx] = weakref.ref(engine)


class GraphedTrainStep:
    def __init__(self, engine, loss_metric, batch, var_weights, scaler=None, warmup: int = 2):
        x, y, self.in_vars, self.out_vars = batch
        if getattr(engine.module, "tensor_par_size", 1) > 1:
            raise NotImplementedError("GraphedTrainStep covers the data-parallel step; tensor-parallel steps (large "
                                      "models, not launch-bound) run eagerly")
        if getattr(engine.module, "patch_size", 2) != 2:
            raise NotImplementedError("GraphedTrainStep with patch_size=%d: graph capture of the step is built and tested for "
                                      "patch_size=2 only; run the step eagerly" % engine.module.patch_size)
        if getattr(engine, "shard_params", False):
            # The parameter-sharding engine is captured in its SINGLE-STREAM form (fsdp_engine.single_stream): per-unit all-gathers,
            # reduce-scatters and pooled-buffer hand-overs in program order on the capturing stream.  Its two-stream form records
            # into a capture but hipStreamEndCapture segfaulted on the result in rounds 3 and 5 (DESIGN 5 lists every fork / join
            # edge of that form; all are event-joined before the step ends, so the runtime, not an unjoined stream, is at fault).
            engine.single_stream(True)
        self.engine, self.loss_metric, self.var_weights, self.scaler = engine, loss_metric, var_weights, scaler
        self.device = engine.device
        if self.device.type == "cuda":
            _claim_salt(engine, self.device)
        self.x = x.to(self.device).clone()           # static input buffers: refill with .copy_ between replays
        self.y = y.to(self.device).clone()
        self.warmup = warmup
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.loss: Optional[torch.Tensor] = None
        self.scale = 1.0
        self.captures = 0

    def _body(self):
        from . import _ops
        _hip.seed_salt(SALT_STEP, add=True)
        _ops.seeds.reset(self._seed_mark)            # the same per-launch seeds at capture time and in the warm-ups
        self.engine.zero_grad()
        loss = training_step((self.x, self.y, self.in_vars, self.out_vars), 0, self.engine, self.device,
                             self.var_weights, self.loss_metric)
        (loss * self.scale).backward()
        self.engine.finish_grad_sync()               # joins the communication stream back into the captured stream
        return loss.detach()

    def capture(self):
        from . import _ops
        # CommStats records timing-enabled events on the capturing streams and reads them back with elapsed_time: a captured event
        # has no timestamp (querying it is invalid), and round 3's segfault in hipStreamEndCapture happened with exactly this
        # combination on the path (profiles/HISTORY_r01_r04.md 6c) -- refuse it instead of handing it to the runtime
        if getattr(self.engine, "comm_stats", None) is not None and not getattr(self, "_allow_comm_stats", False):
            raise RuntimeError("GraphedTrainStep: engine.comm_stats is set -- communication accounting uses timing events and "
                               "cannot run inside a hipGraph capture; unset it (or run the step eagerly)")
        self.engine._o2_capture_live = True
        self.scale = float(self.scaler.get_scale()) if self.scaler is not None else 1.0
        self._seed_mark = _ops.seeds.mark()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                # allocator warm-up and lazy one-time initialisations, uncaptured
            for _ in range(self.warmup):
                self._body()
        torch.cuda.current_stream().wait_stream(side)
        _quiesce_collectives(self.device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode=CAPTURE_ERROR_MODE):
            self.loss = self._body()
        self.captures += 1

    def __call__(self, batch=None):
        """runs one step's zero_grad + forward + loss + backward; returns the (static) loss tensor"""
        if batch is not None:
            self.x.copy_(batch[0], non_blocking=True)
            self.y.copy_(batch[1], non_blocking=True)
        if self.graph is None or (self.scaler is not None and float(self.scaler.get_scale()) != self.scale):
            self.capture()                           # first use, or the loss scale (a captured constant) moved
        self.graph.replay()
        return self.loss
