"""120 config-2 calls (1,024 RSA-2048 signatures, e = 65537, in-field witness) through a pipeline in a FORCED form, into arena regions:
the workload of `rocprofv3 --kernel-trace --stats -- python tools/two_queue_balance_profile.py [two_queue|step] [arena|plain]` for
profiles/r07_two_queue_balance.txt.  The form is forced with h2r_pipeline_set_form where the library has it and with the developer
build's H2R_PIPE_FORM otherwise (attaching a profiler flips the queue probe)."""
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halo2_rsa_amd as H  # noqa: E402
from halo2_rsa_amd import _lib  # noqa: E402

form = sys.argv[1] if len(sys.argv) > 1 else "two_queue"
where = sys.argv[2] if len(sys.argv) > 2 else "arena"
CALLS, B, E, NBUF = 120, 1024, 65537, 3
chip = H.BigIntChip(64, 2048)
pl = chip.pow_fixed_layout(E)
rng = random.Random(7)
N = [rng.getrandbits(2048) | (1 << 2047) | 1 for _ in range(B)]
X = [rng.randrange(n) for n in N]
x, n = chip.assign_integer(X), chip.assign_integer(N)
if where == "arena":
    arena = H.TraceArena.for_pow(chip, E, B, regions=NBUF, candidates=8)
    regions = arena.regions
else:
    regions = [torch.zeros(B * pl.elem_stride, dtype=torch.uint8, device="cuda") for _ in range(NBUF)]
ifs, _ = chip.in_field_layout()
sets = [dict(ws=torch.zeros(chip.workspace_bytes(B, pl.num_mul_mods), dtype=torch.uint8, device="cuda"),
             out=torch.zeros((B, 32), dtype=torch.int64, device="cuda"), status=torch.zeros(B, dtype=torch.uint8, device="cuda"),
             in_field=torch.zeros(B * ifs, dtype=torch.uint8, device="cuda")) for _ in range(NBUF)]
pipe = H.Pipeline(chip, depth=3, side_streams=2)
if hasattr(pipe, "set_form"):
    pipe.set_form(_lib.H2R_PIPE_TWO_QUEUE if form == "two_queue" else _lib.H2R_PIPE_ONE_LAUNCH_STEP)
elif os.environ.get("H2R_PIPE_FORM") is None:
    sys.exit("this library has no h2r_pipeline_set_form: run its -DH2R_DEV_KNOBS build with H2R_PIPE_FORM=0|1")
pi = pipe.info(B)
print("form:", ["one-launch step", "two-queue", "side stream"][pi.record_form], "kept_ms:", getattr(arena, "region_ms", None) if where == "arena" else None)
for k in range(CALLS):
    s = sets[k % NBUF]
    pipe.modpow_public_key(x, E, n, regions[k % NBUF], s["ws"], s["out"], s["status"], s["in_field"])
pipe.join()
torch.cuda.synchronize()
assert not sets[0]["status"].cpu().numpy().any()
print("done", CALLS, "calls")
