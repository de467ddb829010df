"""The data flows of a net's backward (nerfhip_plan_set_bwd_compaction, include/nerfhip.h): their codes and public names, the "auto"
policy that picks among them from the fraction of all-zero d(loss)/d(raw) rows, and the read-back of the two statistics words
{kept, total} a backward over a sample list leaves in its scratch.  What FlexibleNeRFModel.set_backward_compaction,
TrainEngine(backward=...) and the autograd node of the fused render (train_utils._FusedRender) share."""
import torch

NAMES = ("dense", "compact", "recompute", "fused", "fused_compact", "fused_stash")   # (a mode's code is its index)
DENSE, COMPACT, RECOMPUTE, FUSED, FUSED_COMPACT, FUSED_STASH = range(6)
BUILDS_LIST = frozenset((COMPACT, RECOMPUTE, FUSED_COMPACT))   # runs over the list of samples with a non-zero row, writes {kept, total}
FUSED_MODES = frozenset((FUSED, FUSED_COMPACT, FUSED_STASH))   # the one-kernel backward of nets resident in LDS (csrc/mlp64r.hip)
PROBE_EVERY = 50   # "auto": a backward that builds no list reports no fraction, so every 50th pass runs over the list to look again


def parse(value):
    """False / True, an int 0..5 or one of NAMES -> the mode's code; ValueError for anything else ("auto" is a policy, not a mode)."""
    if isinstance(value, bool):
        return int(value)
    if isinstance(value, int) and 0 <= value < len(NAMES):
        return value
    if isinstance(value, str) and value in NAMES:
        return NAMES.index(value)
    raise ValueError("a backward mode is False, True, an int 0..5 or one of %s (got %r)" % (", ".join(map(repr, NAMES)), value))


# A compacted step costs what its gather costs when nothing is dropped (fp32: k_wgrad + 19 %, fp16 pieces + 1 %) and saves the
# dropped fraction of the data and weight gradient; the recomputing mode additionally trades the stash stream of the forward for a
# second forward over the kept samples (pays above ~2/3 dropped rows for the fp16-piece plans, never for fp32): DESIGN.md 3.3-3.4.
# Nets with a fused backward (fp32, 64 wide: csrc/mlp64r.hip) always run it -- over every sample (from the register-image stash,
# mode 5, where the plan has it: 0.70 of the recomputing kernel's time) until the list is known to drop enough of them: 5 % against
# the recomputing mode 3 (the list costs two small launches), 30 % against mode 5 (the list walk recomputes its forward) --, over
# the list from there on.
def choose(frac, f16, fused=0, probe=False):
    """"auto": the mode of a net's next pass.  frac: the last known fraction of all-zero rows (None: unknown); f16: an fp16-piece
    plan; fused: the model's fused_backward_available(); probe: a pass that must report a fraction (runs over the list)."""
    if fused:
        mode = FUSED_COMPACT if (frac is not None and frac >= (0.30 if fused == FUSED_STASH else 0.05)) else (
            FUSED_STASH if fused == FUSED_STASH else FUSED)
    elif frac is None:
        mode = DENSE
    elif f16:
        mode = RECOMPUTE if frac >= 0.72 else (COMPACT if frac >= 0.05 else DENSE)
    else:
        mode = COMPACT if frac >= 0.15 else DENSE
    if probe and mode not in BUILDS_LIST:
        mode = FUSED_COMPACT if mode in FUSED_MODES else COMPACT
    return mode


def fold(prev, kept, total):
    """The zero-row fraction of a pair of statistics words; `prev` for a pair no backward wrote (the workspace is uninitialised
    memory, and a launch of 2^22 or more sample points runs dense without writing them)."""
    return 1.0 - kept / float(total) if (0 <= kept <= total and total > 0) else prev


def stats_words(call, net, ws):
    """The int32 view of {kept, total} of net "coarse" / "fine" in `ws`, the workspace tensor of the render `call` (a
    render_call.RenderCall in a training layout)."""
    so = call.stats_offset(net) // 4
    return ws.view(torch.int32)[so:so + 2]


class StatsReader:
    """The zero-row fractions of a fixed tuple of nets, fed by asynchronous copies of their statistics words into pinned memory
    with ONE event behind each request: polled, never waited for."""

    def __init__(self, nets):
        self.frac = {net: None for net in nets}
        self._host = self._event = self._nets = None

    def __getstate__(self):   # (copy.deepcopy / pickle: the fractions travel, the copy in flight stays behind)
        return dict(self.__dict__, _host=None, _event=None, _nets=None)

    def poll(self):
        """Folds the words of a request that has landed into the fractions."""
        if self._event is not None and self._event.query():
            h = self._host.tolist()
            for k, net in enumerate(self._nets):
                self.frac[net] = fold(self.frac[net], h[2 * k], h[2 * k + 1])
            self._event = None

    def request(self, views, stream):
        """views: (net, its two words on the device) pairs, looked at only if no request is in flight; the copies are enqueued on
        the current stream, the event is recorded on `stream` (the current one)."""
        views = list(views) if self._event is None else []
        if not views:
            return
        if self._host is None:
            self._host = torch.zeros(2 * len(self.frac), dtype=torch.int32).pin_memory()
        for k, (_, words) in enumerate(views):
            self._host[2 * k:2 * k + 2].copy_(words, non_blocking=True)
        self._nets = [net for net, _ in views]
        self._event = torch.cuda.Event()
        self._event.record(stream)
