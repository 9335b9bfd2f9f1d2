"""Diagnostic: standalone stage times of a c2 batch (HIP events, one batch in
flight, as bench.py's stages_standalone_ms), for A/B runs of the band kernel:
LDT_LIBRARY picks the build, LDT_RESIZE_PCT the band count
(LDT_OPT_RESIZE_WAVES_PCT). Prints one line: the resize path taken
(ldt_debug_last_resize) and the mean ms per stage over N batches."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "lance-distributed-training_amd"))
import ldt_amd  # noqa: E402
from ldt_amd import _lib, synth  # noqa: E402

n_batches = int(sys.argv[1]) if len(sys.argv) > 1 else 32
ctx = _lib.get_context(0)
if os.environ.get("LDT_RESIZE_PCT"):
    ctx.set_option(_lib.OPT_RESIZE_WAVES_PCT, int(os.environ["LDT_RESIZE_PCT"]))
ctx.set_option(_lib.OPT_PROFILE, 1)
cells, labels = synth.q90_512(256, seed=1000)
rb = ldt_amd.ResidentBatch(cells, labels)
for _ in range(4):
    rb.decode()
ctx.stage_times(reset=True)
for _ in range(n_batches):
    rb.decode()
st = {k: round(v[0] / max(v[1], 1), 4) for k, v in ctx.stage_times(reset=True).items()}
print("c2 standalone", os.path.basename(os.environ.get("LDT_LIBRARY", "libldt.so")),
      "pct", os.environ.get("LDT_RESIZE_PCT", "default"), "resize_wpg", ctx.lib.ldt_debug_last_resize(ctx.handle), "bands",
      ctx.lib.ldt_debug_last_resize_bands(ctx.handle) if hasattr(ctx.lib, "ldt_debug_last_resize_bands") else "?",
      "stage_ms", st, flush=True)
