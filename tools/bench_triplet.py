"""Times the triplet profile (dmx_engine_triplet, k_triplet) at cfg6 (sparse, 20k x 100k x 16, ~2 000 SNPs per barcode) and cfg3 (dense,
10k x 50k x 32, GP) with C = 2 base pairs per barcode and the T = 4 default share triples, and in the same process, alternating with
it, K1 (the singlet kernel over the same V columns, from dmx_engine_last_kernel_times) as the yardstick.  HIP-event times; the median
of runs 2 to 6.  Slot c of a barcode is (truth + c, truth + c + 1) mod V.  Prints one JSON line per configuration and appends it to
profiles/triplet_bench.jsonl; `per_unit_over_k1` is the time of one (slot, share) over one K1 pass, which DESIGN.md section 19 expects
to be about 1 plus phase 1.

    python tools/bench_triplet.py [--configs 6 3] [--slots 2] [--no-append]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[6, 3])
    ap.add_argument("--slots", type=int, default=2)
    ap.add_argument("--no-append", action="store_true")
    a = ap.parse_args()
    import torch
    import bench
    from demuxlet_amd import build, engine, synth, synth_torch, triplet
    build.build()
    dev = torch.device("cuda", 0)
    shares = triplet.default_shares()
    for cfg_id in a.configs:
        cfg = bench.CONFIGS[cfg_id]
        B, S, V = cfg["B"], cfg["S"], cfg["V"]
        rng = np.random.default_rng(0x7B1E0000 + cfg_id)
        raw, g = bench.genotype_matrix(engine, synth, rng, S, V, cfg["field"])
        dosage = torch.from_numpy(np.clip(raw.alleles, 0, 1).sum(axis=2).astype(np.float32)).to(dev)
        dp = synth_torch.make_device_pileup(dosage, B, cfg["delta"], cfg["rbar"], seed=0x7B1E + 1000 * cfg_id, device=dev)
        t0 = dp.truth[:, 0].cpu().numpy().astype(np.int32)
        base = np.stack([np.stack([(t0 + c) % V, (t0 + c + 1) % V], axis=1) for c in range(a.slots)], axis=1).astype(np.int32)
        d_base = torch.from_numpy(base).to(dev)
        torch.cuda.synchronize()
        e = engine.Engine(V, cfg["alphas"], 0.5)
        e.set_genotypes(g)
        e.set_pileup_struct(dp.as_struct(), keep=dp)
        C, T = a.slots, len(shares)
        trp, k1 = [], []
        for i in range(6):
            rq = engine.capi.TripletRequest(B, engine.capi.DMX_MEM_DEVICE, int(d_base.data_ptr()), C, T, S, 0, shares.ctypes.data)
            engine.check(e._L.dmx_engine_triplet(e._h, engine.C.byref(rq)))       # the profile stays on the device: only the kernel is timed
            trp.append(e.triplet_info()["kernel_ms"])
            e.run_singlet(); e.sync()
            k1.append(float(e.kernel_times().singlet_ms))
        trp, k1 = trp[1:], k1[1:]
        mt, mk = statistics.median(trp), statistics.median(k1)
        row = dict(config=cfg_id, B=B, S=S, V=V, pairs=dp.n_pairs, reads=dp.n_reads, n_base=C, n_shares=T, reps=len(trp), triplet_ms=round(mt, 3),
                   triplet_ms_min=round(min(trp), 3), triplet_ms_max=round(max(trp), 3), k1_ms=round(mk, 3), k1_ms_min=round(min(k1), 3),
                   k1_ms_max=round(max(k1), 3), ratio=round(mt / mk, 3), per_unit_over_k1=round(mt / mk / (C * T), 3))
        line = json.dumps(row)
        print(line, flush=True)
        if not a.no_append:
            with open(ROOT / "profiles" / "triplet_bench.jsonl", "a") as f:
                f.write(line + "\n")
        e.close()
        del dp, dosage, d_base
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
