"""How far can this pool's calls be trusted at this depth?  In-silico doublets and thinned barcodes from the pool's own droplets.

    python -m demuxlet_amd.simulate --pileup <x>.pileup.txt --out <prefix> [--best <x>.best] [--min-prb P] [--n N] [--depth F ...]
        [--share A ...] [--seed S] [--alpha A ...] [--fast] [--gpu G]

The reads of two called singlets are merged and thinned on the GPU (Engine.compose), the unchanged demultiplexing
pass runs on the result, and what comes out is counted.  For every depth fraction F and share A, N barcodes of each of three kinds:

    HET   two parents of different donors, kept at min(1, 2 A F) and min(1, 2 (1 - A) F): a heterotypic doublet at F times the depth
          of a doublet of two average cells, the first donor contributing a share A of the reads;
    HOM   two different parents of the same donor, same fractions: a homotypic doublet, which no genotype method can see;
    SNG   one parent kept at F: the negative control at matched depth.

Outputs: <prefix>.sim.best/.single/.sing2 (the ordinary files for the simulated barcodes SIM0000000, SIM0000001, ...),
<prefix>.sim.recipe.tsv (what was drawn), <prefix>.sim.tsv (one row per simulated barcode with its call and whether it is right) and
<prefix>.power.tsv (rates per kind, depth and share, and the pool's total doublet rate behind the observed heterotypic one).

Caveats.  The parents' donors are CALLS of the plain pass (SNG- rows with PRB.SNG1 >= --min-prb), not truth: a wrong call puts a
wrong label on everything made from that barcode.  At most two parents; no ambient RNA is added; a real doublet's capture
efficiency (two cells in a droplet rarely yield twice the reads) is not modelled — `--depth` is the knob for that.  A parent that is
itself an undetected doublet makes a triplet.  The rd_* counters of the simulated barcodes are synthetic (the kept reads)."""
from __future__ import annotations

import argparse
import os
import sys
from typing import Optional, Sequence

import numpy as np

from . import ambient, capi, engine, refine

KINDS = ("HET", "HOM", "SNG")
KIND_HET, KIND_HOM, KIND_SNG = 0, 1, 2
KEEP_ALL = 1 << 32
SIM_HEADER = "BARCODE\tKIND\tDEPTH\tSHARE\tPARENT1\tPARENT2\tDONOR1\tDONOR2\tN.SNP\tN.READ\tBEST\tOK\n"
POWER_HEADER = "KIND\tDEPTH\tSHARE\tN\tN.SNG\tN.DBL\tN.AMB\tN.OK\tRATE\tMED.SNP\tMED.READ\n"
RECIPE_HEADER = "BARCODE\tKIND\tDEPTH\tSHARE\tCELL1\tCELL2\tKEEP1\tKEEP2\n"


def sim_name(k: int) -> str:
    """Zero-padded, so that the writers' byte-wise barcode order is the recipe's order and chunks concatenate."""
    return f"SIM{k:07d}"


def threshold(fraction: float) -> int:
    """A kept fraction as the composer's threshold: round(fraction * 2^32), fractions capped at 1."""
    return int(round(min(1.0, max(0.0, float(fraction))) * KEEP_ALL))


def check_fractions(depths, shares):
    d = [float(x) for x in depths]
    s = [float(x) for x in shares]
    if not d or any(not 0.0 < x <= 1.0 for x in d):
        raise ValueError("depth fractions must be in (0, 1]")
    if not s or any(not 0.0 < x < 1.0 for x in s):
        raise ValueError("shares must be in (0, 1)")
    return d, s


def draw_recipe(assign, depths, shares, n: Optional[int], seed: int) -> dict:
    """The recipe for parents assign[cell] = donor (-1: not a parent).  Deterministic in (assign, depths, shares, n, seed).  Rows are
    ordered by depth, share, kind (HET, HOM, SNG); a kind that cannot be drawn (HET with one donor, HOM when no donor has two parents)
    is left out.  Returns arrays kind, depth, share, parent[.][2], keep[.][2] (uint64), donor[.][2]."""
    depths, shares = check_fractions(depths, shares)
    assign = np.asarray(assign, dtype=np.int64)
    parents = np.flatnonzero(assign >= 0)
    if len(parents) == 0:
        raise ValueError("no parent barcodes: the .best has no singlet call that passes --min-prb")
    if n is None:
        n = min(2000, len(parents))
    if n < 1:
        raise ValueError("n must be >= 1")
    rng = np.random.default_rng(seed)
    donors = np.unique(assign[parents])
    by_donor = {int(d): parents[assign[parents] == d] for d in donors}
    hom_parents = np.concatenate([p for p in by_donor.values() if len(p) >= 2]) if any(len(p) >= 2 for p in by_donor.values()) else np.zeros(0, np.int64)
    kind, depth, share, par, keep, don = [], [], [], [], [], []
    for f in depths:
        for a in shares:
            k0, k1 = threshold(2.0 * a * f), threshold(2.0 * (1.0 - a) * f)
            if len(donors) >= 2:
                for _ in range(n):
                    p = int(parents[rng.integers(len(parents))])
                    others = parents[assign[parents] != assign[p]]
                    q = int(others[rng.integers(len(others))])
                    kind.append(KIND_HET); par.append((p, q)); keep.append((k0, k1)); don.append((int(assign[p]), int(assign[q])))
                    depth.append(f); share.append(a)
            if len(hom_parents):
                for _ in range(n):
                    p = int(hom_parents[rng.integers(len(hom_parents))])
                    same = by_donor[int(assign[p])]
                    same = same[same != p]
                    q = int(same[rng.integers(len(same))])
                    kind.append(KIND_HOM); par.append((p, q)); keep.append((k0, k1)); don.append((int(assign[p]), int(assign[q])))
                    depth.append(f); share.append(a)
            for _ in range(n):
                p = int(parents[rng.integers(len(parents))])
                kind.append(KIND_SNG); par.append((p, -1)); keep.append((threshold(f), 0)); don.append((int(assign[p]), -1))
                depth.append(f); share.append(a)
    return dict(kind=np.array(kind, dtype=np.int32), depth=np.array(depth), share=np.array(share), parent=np.array(par, dtype=np.int32).reshape(-1, 2),
                keep=np.array(keep, dtype=np.uint64).reshape(-1, 2), donor=np.array(don, dtype=np.int32).reshape(-1, 2), n=n)


def chunk_recipe(pl: engine.HostPileup, parent: np.ndarray, max_bytes: int):
    """Consecutive row ranges whose composed pileup (bounded by the parents' sizes) stays below max_bytes; a row alone always fits."""
    npair = np.diff(np.asarray(pl.cell_pair_off, dtype=np.int64)); nread = np.diff(np.asarray(pl.cell_read_off, dtype=np.int64))
    cost = np.zeros(len(parent), dtype=np.int64)
    for s in range(2):
        c = parent[:, s]
        ok = c >= 0
        cost[ok] += 8 * npair[c[ok]] + nread[c[ok]] + 16
    out, k0, acc = [], 0, 0
    for k in range(len(parent)):
        if k > k0 and acc + int(cost[k]) > max_bytes:
            out.append((k0, k)); k0, acc = k, 0
        acc += int(cost[k])
    if len(parent) > k0:
        out.append((k0, len(parent)))
    return out


def row_ok(kind: int, donor, best: str, sng1: int, dbl1: int, dbl2: int) -> bool:
    """HET: called DBL- with exactly its two donors, in either order.  HOM, SNG: called SNG- of its donor."""
    if kind == KIND_HET:
        return best.startswith("DBL-") and {int(dbl1), int(dbl2)} == {int(donor[0]), int(donor[1])}
    return best.startswith("SNG-") and int(sng1) == int(donor[0])


def write_recipe_tsv(path: str, rc: dict) -> None:
    with open(path, "w") as f:
        f.write(RECIPE_HEADER)
        for k in range(len(rc["kind"])):
            f.write(f"{sim_name(k)}\t{KINDS[rc['kind'][k]]}\t{rc['depth'][k]:g}\t{rc['share'][k]:g}\t{rc['parent'][k, 0]}\t{rc['parent'][k, 1]}\t"
                    f"{int(rc['keep'][k, 0])}\t{int(rc['keep'][k, 1])}\n")


def write_sim_tsv(path: str, rc: dict, barcodes: Sequence[str], sample_ids: Sequence[str], n_snp, n_read, rows: ambient.BestRows) -> np.ndarray:
    """<prefix>.sim.tsv; returns OK per row.  A simulated barcode without a `.best` row (no covered SNP left) has BEST = NA and is not OK."""
    ok = np.zeros(len(rc["kind"]), dtype=bool)
    with open(path, "w") as f:
        f.write(SIM_HEADER)
        for k in range(len(rc["kind"])):
            p, d = rc["parent"][k], rc["donor"][k]
            best = rows.best[k]
            ok[k] = bool(best) and row_ok(int(rc["kind"][k]), d, best, rows.sng1[k], rows.dbl1[k], rows.dbl2[k])
            f.write(f"{sim_name(k)}\t{KINDS[rc['kind'][k]]}\t{rc['depth'][k]:g}\t{rc['share'][k]:g}\t{barcodes[p[0]]}\t"
                    f"{barcodes[p[1]] if p[1] >= 0 else 'NA'}\t{sample_ids[d[0]]}\t{sample_ids[d[1]] if d[1] >= 0 else 'NA'}\t"
                    f"{int(n_snp[k])}\t{int(n_read[k])}\t{best if best else 'NA'}\t{int(ok[k])}\n")
    return ok


def pool_estimate(real_best: ambient.BestRows, assign, het_rate_full: Optional[float]) -> dict:
    """The pool's total doublet rate behind the observed one: observed DBL share of the real `.best` / (HET sensitivity at depth 1 x
    heterotypic fraction), the heterotypic fraction 1 - sum p_d^2 from the donors' shares p_d of the parents."""
    called = [b for b in real_best.best if b]
    obs = sum(b.startswith("DBL-") for b in called) / len(called) if called else float("nan")
    a = np.asarray(assign)
    a = a[a >= 0]
    p = np.bincount(a) / len(a) if len(a) else np.zeros(1)
    het_frac = float(1.0 - np.sum(p * p))
    sens = float("nan") if het_rate_full is None else float(het_rate_full)
    est = obs / (sens * het_frac) if sens > 0 and het_frac > 0 else float("nan")
    return dict(obs_dbl=obs, het_sens=sens, het_frac=het_frac, est_dbl=est)


def power_table(rc: dict, best: Sequence[str], ok, n_snp, n_read):
    """One entry per (kind, depth, share) in kind-major order: dicts with the counts, the OK rate and the median N.SNP / N.READ."""
    out = []
    ok = np.asarray(ok, dtype=bool)
    for kd in range(3):
        seen = []
        for k in np.flatnonzero(rc["kind"] == kd):
            key = (float(rc["depth"][k]), float(rc["share"][k]))
            if key not in seen:
                seen.append(key)
        for f, a in seen:
            idx = np.flatnonzero((rc["kind"] == kd) & (rc["depth"] == f) & (rc["share"] == a))
            b = [best[k] for k in idx]
            n_sng = sum(x.startswith("SNG-") for x in b); n_dbl = sum(x.startswith("DBL-") for x in b)
            out.append(dict(kind=KINDS[kd], depth=f, share=a, n=len(idx), n_sng=n_sng, n_dbl=n_dbl, n_amb=len(idx) - n_sng - n_dbl,
                            n_ok=int(ok[idx].sum()), rate=float(ok[idx].mean()), med_snp=float(np.median(np.asarray(n_snp)[idx])),
                            med_read=float(np.median(np.asarray(n_read)[idx]))))
    return out


def het_rate_at_full_depth(table) -> Optional[float]:
    het = [r for r in table if r["kind"] == "HET" and r["depth"] == 1.0]
    if not het:
        return None
    return min(het, key=lambda r: abs(r["share"] - 0.5))["rate"]


def write_power_tsv(path: str, table, pool: dict) -> None:
    """<prefix>.power.tsv: the HET rows, the pool-level estimate (a `#POOL` line), then the HOM and SNG rows.  N.AMB counts every barcode
    that is neither SNG- nor DBL- (AMB- calls and barcodes without a row), so N.SNG + N.DBL + N.AMB = N."""
    def row(r):
        return (f"{r['kind']}\t{r['depth']:g}\t{r['share']:g}\t{r['n']}\t{r['n_sng']}\t{r['n_dbl']}\t{r['n_amb']}\t{r['n_ok']}\t{r['rate']:.4f}\t"
                f"{r['med_snp']:g}\t{r['med_read']:g}\n")
    with open(path, "w") as f:
        f.write(POWER_HEADER)
        for r in table:
            if r["kind"] == "HET":
                f.write(row(r))
        f.write("#POOL\tOBS.DBL\tHET.SENS\tHET.FRAC\tEST.DBL\n")
        f.write(f"#POOL\t{pool['obs_dbl']:.4f}\t{pool['het_sens']:.4f}\t{pool['het_frac']:.4f}\t{pool['est_dbl']:.4f}\n")
        for r in table:
            if r["kind"] != "HET":
                f.write(row(r))


def _append(dst: str, src: str, first: bool) -> None:
    with open(src) as s, open(dst, "w" if first else "a") as d:
        head = s.readline()
        if first:
            d.write(head)
        for line in s:
            d.write(line)
    os.remove(src)


def simulate_run(pileup: engine.HostPileup, g: np.ndarray, sample_ids: Sequence[str], out_prefix: str, barcodes: Sequence[str],
                 best: Optional[str] = None, min_prb: float = 0.99, n: Optional[int] = None, depths: Sequence[float] = (1.0, 0.5, 0.25, 0.1),
                 shares: Sequence[float] = (0.5,), seed: int = 0, alphas: Sequence[float] = (0.0, 0.5), device: int = 0,
                 mode: int = capi.DMX_MODE_STRICT, max_bytes: int = 1 << 30, **demuxlet_run_kwargs) -> dict:
    """Draw the recipe from the singlets of `best` (without it the plain pass writes <out_prefix>.best/.single/.sing2 first), compose the
    barcodes on the device, run the unchanged demuxlet_run on them (same g, alphas and mode) and write the outputs named in the module
    docstring.  The recipe is composed in chunks of at most max_bytes; the result does not depend on the chunking.  Returns a dict with
    the recipe, the calls, OK per row, the power table and the pool estimate."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    pl = pileup
    if g.ndim != 3 or g.shape[0] != pl.n_snps or g.shape[1] != len(sample_ids) or g.shape[2] != 3:
        raise ValueError(f"genotype matrix {g.shape} for {pl.n_snps} SNPs and {len(sample_ids)} samples")
    check_fractions(depths, shares)
    if best is None:
        engine.demuxlet_run(pl, g, sample_ids, alphas, out_prefix, barcodes=barcodes, device=device, mode=mode, **demuxlet_run_kwargs)
        best = out_prefix + ".best"
    assign = refine.assignments_from_best(best, sample_ids, barcodes, min_prb)
    rc = draw_recipe(assign, depths, shares, n, seed)
    write_recipe_tsv(out_prefix + ".sim.recipe.tsv", rc)
    K = len(rc["kind"])
    names = [sim_name(k) for k in range(K)]
    n_snp = np.zeros(K, dtype=np.int32); n_read = np.zeros(K, dtype=np.int32)
    compose_ms = 0.0
    eng = engine.Engine(len(sample_ids), alphas, device=device, mode=mode)
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        for ci, (k0, k1) in enumerate(chunk_recipe(pl, rc["parent"], max_bytes)):
            inf = eng.compose(rc["parent"][k0:k1], rc["keep"][k0:k1], seed, index_base=k0)
            compose_ms += inf["count_ms"] + inf["scan_ms"] + inf["fill_ms"]
            po, ro = eng.composed_offsets()
            n_snp[k0:k1] = np.diff(po); n_read[k0:k1] = np.diff(ro)
            kept = np.ascontiguousarray(n_read[k0:k1])            # synthetic RD.TOTL / RD.PASS / RD.UNIQ: the kept reads
            st = eng.composed_pileup()
            st.rd_totl = st.rd_pass = st.rd_uniq = kept.ctypes.data
            part = f"{out_prefix}.sim.part{ci}"
            engine.demuxlet_run(st, g, sample_ids, alphas, part, barcodes=names[k0:k1], device=device, mode=mode, **demuxlet_run_kwargs)
            for ext in (".best", ".single", ".sing2"):
                _append(out_prefix + ".sim" + ext, part + ext, ci == 0)
    finally:
        eng.close()
    rows = ambient.read_best_rows(out_prefix + ".sim.best", sample_ids, names)
    ok = write_sim_tsv(out_prefix + ".sim.tsv", rc, barcodes, sample_ids, n_snp, n_read, rows)
    table = power_table(rc, rows.best, ok, n_snp, n_read)
    pool = pool_estimate(ambient.read_best_rows(best, sample_ids, barcodes), assign, het_rate_at_full_depth(table))
    write_power_tsv(out_prefix + ".power.tsv", table, pool)
    return dict(assign=assign, recipe=rc, names=names, best=rows.best, ok=ok, n_snp=n_snp, n_read=n_read, table=table, pool=pool,
                compose_ms=compose_ms)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.simulate",
                                 description="detection power at this pool's depth from in-silico doublets and thinned barcodes")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.sim.best/.single/.sing2, .sim.tsv, .sim.recipe.tsv, .power.tsv")
    ap.add_argument("--best", help="a .best of this pileup: its singlets are the parents (default: run the demultiplexing pass first)")
    ap.add_argument("--min-prb", type=float, default=0.99, help="parents are the SNG- calls with PRB.SNG1 >= this (default 0.99)")
    ap.add_argument("--n", type=int, help="barcodes per kind, depth and share (default: min(2000, parents))")
    ap.add_argument("--depth", type=float, nargs="+", default=[1.0, 0.5, 0.25, 0.1], help="depth fractions in (0, 1] (default 1 0.5 0.25 0.1)")
    ap.add_argument("--share", type=float, nargs="+", default=[0.5], help="read share of a doublet's first parent, in (0, 1) (default 0.5)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="doublet grid of the demultiplexing passes (default 0 0.5)")
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST for the demultiplexing passes")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    if not 0.0 <= a.min_prb <= 1.0:
        ap.error("--min-prb must be in [0, 1]")
    if a.n is not None and a.n < 1:
        ap.error("--n must be >= 1")
    if a.seed < 0:
        ap.error("--seed must be >= 0")
    try:
        a.depth, a.share = check_fractions(a.depth, a.share)
    except ValueError as ex:
        ap.error(str(ex))
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    r = simulate_run(d.pileup, d.g, d.sample_ids, a.out, d.barcodes, best=a.best, min_prb=a.min_prb, n=a.n, depths=a.depth, shares=a.share,
                     seed=a.seed, alphas=a.alpha, device=a.gpu, mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT)
    for t in r["table"]:
        print(f"{t['kind']} depth {t['depth']:g} share {t['share']:g}: {t['n_ok']}/{t['n']} right", file=sys.stderr)
    print(f"pool: observed DBL {r['pool']['obs_dbl']:.4f}, estimated total doublet rate {r['pool']['est_dbl']:.4f}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
