"""profiles/EXPERIMENTS.md, "Simulation study": ops.rtt_score against the parent's path (a loop of lr_rtt_summary(pooled) over the groups' slices, from the parent commit's
library), HIP events, one warm-up, seven timed, median; then the achieved read bandwidth"""
import ctypes as C, json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from literate_amd import ops, _hip, simstudy

out = {}
PARENT = os.environ.get("LR_PARENT_LIB", "")          # libliterate_hip.so built from the parent commit
assert os.path.exists(PARENT), "LR_PARENT_LIB: the parent commit's libliterate_hip.so (the path it is compared against)"
nb = 40          # two birth shifts and one death shift over 40 unit bins
sc = np.stack([np.where(np.arange(nb) < 15, 0.2, np.where(np.arange(nb) < 30, 0.4, 0.15)), np.where(np.arange(nb) < 25, 0.1, 0.25)])
t0 = time.time()
res = simstudy.run(sc, 256, chains_per_rep=4, n_iter=200000, s_freq=200, seed=11, keep_trace=True, verbose=True)
out["study_run_seconds"] = dict(res.seconds, total=time.time() - t0)
out["kept"] = int(res.kept.size)
trace = res.trace
S, Cn = 1000, trace.shape[1]
a, b, burnin = 0.0, nb + 0.5, 0.2
print("trace", tuple(trace.shape), "kept", res.kept.size)
if Cn < 1024:          # (dropped replicates: fill up with copies so the shapes are the issue's)
    trace = torch.cat([trace, trace[:, :1024 - Cn]], dim=1).contiguous()
    Cn = 1024
parent = C.CDLL(os.path.abspath(PARENT))
parent.lr_rtt_summary_workspace_bytes.restype = C.c_int64
parent.lr_rtt_summary_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32]
parent.lr_rtt_summary.restype = C.c_int32
parent.lr_rtt_summary.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_int64, C.c_void_p]


def timed(fn, reps=7):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [round(m, 3) for m in ms]


truth = torch.as_tensor(sc, device="cuda")
for cpg in (4, 1):
    G = Cn // cpg
    key = "%dx%dx%dx%d" % (G, cpg, S, nb)
    tr_full = truth[None].expand(G, -1, -1).contiguous()
    new_ms, new_all = timed(lambda: ops.rtt_score(trace, S, cpg, a, b, truth=tr_full, burnin=burnin))
    plain_ms, _ = timed(lambda: ops.rtt_score(trace, S, cpg, a, b, burnin=burnin))
    got = ops.rtt_score(trace, S, cpg, a, b, truth=tr_full, burnin=burnin)
    # the parent's path: pre-sliced contiguous inputs, one workspace, its outputs side by side
    slices = [trace[:, g * cpg:(g + 1) * cpg].contiguous() for g in range(G)]
    wsb = int(parent.lr_rtt_summary_workspace_bytes(S, cpg, a, b, burnin, 1))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    rates, freq, kc = torch.empty_like(got.rates), torch.empty_like(got.shift_freq), torch.empty_like(got.k_counts)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def loop():
        for g in range(G):
            rc = parent.lr_rtt_summary(C.c_void_p(slices[g].data_ptr()), S, cpg, a, b, burnin, 1, C.c_void_p(rates[g].data_ptr()),
                                       C.c_void_p(freq[g].data_ptr()), C.c_void_p(kc[g].data_ptr()), C.c_void_p(ws.data_ptr()), wsb, stream)
            assert rc == 0, rc
    old_ms, old_all = timed(loop)
    torch.cuda.synchronize()
    same = bool(torch.equal(rates, got.rates) and torch.equal(freq, got.shift_freq) and torch.equal(kc, got.k_counts))
    n = cpg * (S - int(burnin * S))
    unique = G * n * _hip.LR_TRACE_W * 8
    out[key] = dict(rtt_score_ms=new_ms, rtt_score_all=new_all, rtt_score_no_truth_ms=plain_ms, parent_loop_ms=old_ms, parent_loop_all=old_all,
                    parent_workspace_bytes=wsb, bit_identical=same, kept_trace_bytes=unique,
                    read_GBps_unique=unique / (plain_ms * 1e-3) / 1e9, read_GBps_rows_times_bins=unique * nb / (plain_ms * 1e-3) / 1e9)
    print(key, json.dumps(out[key]))
    del slices
json.dump(out, open(os.environ.get("LR_SCORE_JSON", "score_experiments.json"), "w"), indent=1)
print("coverage birth", res.score[0, :, 1].round(3).tolist())
print("coverage death", res.score[1, :, 1].round(3).tolist())
print("shifts", {k: (v.tolist() if hasattr(v, "tolist") else [np.asarray(x).tolist() for x in v]) for k, v in res.shifts.items() if k not in ("reported", "two_ln_bf", "k_mode")})
