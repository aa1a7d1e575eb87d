"""N-rank RCCL check of the gradient exchange (needs >= 2 GPUs — never run by this build, no multi-GPU node was available):

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29612 tools/rccl_two_rank_check.py

Every rank trains the same model on ITS shard of a fixed synthetic batch for a few captured steps under each gradient-exchange layout
    A  fp32 wire, collectives between the graphs on torch.distributed's communicator   (the default)
    B  fp32 wire, collectives captured into the step's graph (VMASR_GRAPH_COLLECTIVES=1: RCCL's C API + CollectiveWatchdog)
    C  bf16 wire for the MPD gradient (VMASR_GRAD_COMM=mpd-bf16), between the graphs
and checks: (1) after every layout all ranks hold IDENTICAL weights (the all-reduce really averaged); (2) B reproduces A's losses and
weights to fp32 rounding (same arithmetic, different scheduling); (3) C stays within 2e-2 of A's losses (the bf16 wire is a numerics
change: 3e-4 ... 9e-4 on one step's losses).  On ONE GPU: FAKE_WORLD=2 python tools/rccl_two_rank_check.py — a 1-rank RCCL group with the trainer told that world = 2: the collectives are the
identity and (1)-(3) hold trivially; that run only shows that the script and all three code paths execute (tests/test_multigpu.py).  Exit code 0 = all checks passed on every rank."""
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
os.environ.setdefault("TENSILE_STREAMK_DATA_PARALLEL", "1")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
os.environ.setdefault("VMASR_STEP_VARIANT", "lane:0.75")          # the same captured layout in every run
if "RANK" not in os.environ:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", "29613"), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import bench  # noqa: E402
from vm_asr_amd.trainer import init_distributed, unwrap  # noqa: E402

rank, local, world = init_distributed()
dev = torch.device("cuda", local % torch.cuda.device_count())
torch.cuda.set_device(dev)
FAKE = world == 1 and os.environ.get("FAKE_WORLD") == "2"     # one GPU: a 1-rank RCCL group, the trainer told that world = 2 (collectives = identity)
if FAKE:
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
STEPS = int(os.environ.get("STEPS", "4"))
cfg = bench.make_config("vm_asr_48k_MPD", int(os.environ.get("BATCH", "2")))
batches = [bench.synth_batch(cfg, dev, 1000 * s + rank) for s in range(STEPS)]      # rank-local shards, the same in every layout


def run(tag, env):
    for k in ("VMASR_GRAPH_COLLECTIVES", "VMASR_GRAD_COMM"):
        os.environ.pop(k, None)
    os.environ.update(env)
    tr = bench.build_trainer(cfg, dev, amp=True, capturable=True)        # seeded construction: identical initial weights on every rank
    if FAKE:
        tr.world = tr.grads.world = 2
    for m in tr.models.values():
        m.train()
    tr.train_step(*batches[0])
    ok = tr.enable_graphs(batches[0], warmup=2)                           # (state restored: every layout starts from the initial weights)
    assert ok, getattr(tr, "graph_error", None)
    torch.manual_seed(7 + rank)
    torch.cuda.manual_seed_all(7 + rank)
    losses = []
    for b in batches:
        _, logs = tr.train_step(*b)
        losses.append(torch.stack([logs["total_loss"].float(), logs["total_disc_loss"].float()]))
    torch.cuda.synchronize()
    w = torch.cat([p.detach().flatten().float() for m in tr.models.values() for p in unwrap(m).parameters()])
    # (1) identical weights on all ranks
    lo, hi = w.clone(), w.clone()
    if world > 1:
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    spread = float((hi - lo).abs().max())
    info = dict(in_graph=bool(tr._graphed.collectives_in_graph), mpd_wire=str(tr.grads.comm_dtype("mpd")), spread=spread)
    if rank == 0:
        print(f"[{tag}] {info} losses {[ [round(float(v), 4) for v in l] for l in losses]}", flush=True)
    del tr
    torch.cuda.empty_cache()
    return torch.stack(losses), w, info


A = run("A fp32 wire, between the graphs", {})
B = run("B fp32 wire, in the graph", {"VMASR_GRAPH_COLLECTIVES": "1"})
C = run("C bf16 MPD wire, between the graphs", {"VMASR_GRAD_COMM": "mpd-bf16"})
fail = []
for tag, r in (("A", A), ("B", B), ("C", C)):
    if r[2]["spread"] != 0.0:
        fail.append(f"{tag}: ranks hold different weights (max spread {r[2]['spread']:.3e})")
if (world > 1 or FAKE) and not B[2]["in_graph"]:
    fail.append("B: the collectives were not captured into the graph")
rel = lambda x, y: float(((x - y).abs() / y.abs().clamp_min(1.0)).max())      # noqa: E731
# B vs A: the same arithmetic — but default-mode atomics and bf16 autocast move single steps by ~1e-3 (profiles/r06_determinism_hunt.md)
if rel(B[0], A[0]) > 2e-2:
    fail.append(f"B: losses differ from A by {rel(B[0], A[0]):.3e}")
if rel(C[0], A[0]) > 2e-2:
    fail.append(f"C: losses differ from A by {rel(C[0], A[0]):.3e}")
dw = lambda x, y: float((x - y).norm() / y.norm())                             # noqa: E731
if rank == 0:
    print(f"world {world}: B vs A losses {rel(B[0], A[0]):.3e}, weights {dw(B[1], A[1]):.3e};  C vs A losses {rel(C[0], A[0]):.3e}, weights {dw(C[1], A[1]):.3e}")
    print("FAILED: " + "; ".join(fail) if fail else "all checks passed")
flag = torch.tensor([1.0 if fail else 0.0], device=dev)
if world > 1:
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)
if dist.is_initialized():
    dist.destroy_process_group()
sys.exit(1 if flag.item() else 0)
