"""Demultiplexing of partly genotyped pools: Vk donors of the pool are in the VCF, M more are not.

The known donors' columns stay fixed; M "unknown" donors are learned by the EM of section 13 in R restarts that share the known columns.
One engine holds V = Vk + R * M columns, [known | restart 0's M | ... | restart R-1's M], so K1 scores the known columns once per
iteration rather than once per restart:
  E-step   K1 (Engine.run_singlet), then cluster_estep_known: a softmax over the Vk + M components of each (barcode, restart); the free
           weights stay on the device, the per-restart LL and the column sums come back.
  M-step   cluster_mstep_window pools the free weights into gp' for the R * M free columns (section 13's arithmetic, prior q) and writes
           it beside the known rows; the result becomes K1's matrix by pointer.
Initialisation: K1 once over [known | q] (q the Hardy-Weinberg prior as one column); a barcode whose best known llk is at least its llk
against q starts on that known donor, every other barcode on a free column drawn at random per restart.  The restart of highest LL
wins; the unchanged `demuxlet_run` writes <prefix>.best/.single/.sing2 over [known | the winner's M columns] with sample ids
known ids + UNK0 .. UNK{M-1}, so doublets of a known and an unknown donor come out of its grid.  Each round r >= 1 refines every column
from the previous round's singlets (known columns against their VCF rows, unknown ones against q) and runs again to <prefix>.r<r>.*.

    python -m demuxlet_amd.partial --pileup <x>.pileup.txt --n-unknown M --out <prefix> [--restarts R] [--seed S] [--max-iter N]
        [--tol T] [--floor F] [--min-snp M] [--alpha A ...] [--rounds N] [--match] [--fast] [--gpu G]

reads the dump that `demuxlet --pileup-only` writes; its genotyped samples are the known donors."""
from __future__ import annotations

import argparse
import sys
from typing import List, Optional, Sequence

import numpy as np

from . import capi, cluster, engine, refine


def unknown_ids(n_unknown: int) -> List[str]:
    return [f"UNK{m}" for m in range(n_unknown)]


def check_args(n_known: int, n_unknown: int, restarts: int, known_ids: Sequence[str], max_iter: int, tol: float, floor: float,
               n_cells: int, n_pairs: int) -> None:
    """The error paths of partial_run, before any device work."""
    if n_known < 1:
        raise ValueError("no genotyped donors: a pool without known donors is demultiplexed by demuxlet_amd.cluster")
    if n_unknown < 1:
        raise ValueError(f"--n-unknown {n_unknown}: at least 1 (a pool with every donor genotyped is demultiplexed by demuxlet_run)")
    if restarts < 1:
        raise ValueError(f"--restarts {restarts}: at least 1")
    if n_known + restarts * n_unknown > cluster.MAX_COLUMNS:
        raise ValueError(f"{n_known} known + {restarts} restarts x {n_unknown} unknown = {n_known + restarts * n_unknown} columns; one engine "
                         f"holds at most {cluster.MAX_COLUMNS}")
    if len(known_ids) != n_known:
        raise ValueError(f"{len(known_ids)} sample ids for {n_known} known genotype columns")
    clash = sorted(set(known_ids) & set(unknown_ids(n_unknown)))
    if clash:
        raise ValueError(f"known sample id {clash[0]} collides with the unknown donors' ids UNK0 .. UNK{n_unknown - 1}")
    if len(set(known_ids)) != len(known_ids):
        raise ValueError("known sample ids must be distinct")
    if max_iter < 1:
        raise ValueError(f"--max-iter {max_iter}: at least 1")
    if not (tol >= 0.0) or not (floor >= 0.0):
        raise ValueError("--tol and --floor must be >= 0")
    if n_cells < 1 or n_pairs == 0:
        raise ValueError(f"empty pileup: {n_cells} barcodes, {n_pairs} covered (barcode, SNP) pairs")


def check_init_labels(labels, n_cells: int, n_known: int, n_unknown: int) -> np.ndarray:
    """init_labels as int32 [R][B], entries in [-1, Vk + M): a known donor j < Vk, a free column Vk + m, or -1 (no weight)."""
    return cluster.check_init_labels(labels, n_cells, n_known + n_unknown)


def initial_labels(llk_known: np.ndarray, llk_q: np.ndarray, seed: int, restarts: int, n_unknown: int) -> np.ndarray:
    """labels[R][B] of the seeded start: a barcode whose best known llk (the lowest donor on a tie) is >= its llk against the prior q
    is "explained" and starts on that donor in every restart; the others get Vk + m, m drawn per restart as
    np.random.default_rng(seed).integers(0, M, size=<number of the others>)."""
    llk_known = np.asarray(llk_known, dtype=np.float64)
    B, Vk = llk_known.shape
    best = np.argmax(llk_known, axis=1)
    explained = llk_known[np.arange(B), best] >= np.asarray(llk_q, dtype=np.float64)
    rest = np.flatnonzero(~explained)
    rng = np.random.default_rng(seed)
    lab = np.empty((restarts, B), dtype=np.int32)
    for r in range(restarts):
        lab[r] = best
        lab[r, rest] = Vk + rng.integers(0, n_unknown, size=rest.size)
    return lab


def random_labels(seed: int, restarts: int, n_cells: int, n_known: int, n_unknown: int) -> np.ndarray:
    """labels[R][B] of a plain random start (every barcode on a random free column; section 13's start), for comparison."""
    return (n_known + cluster.initial_labels(seed, restarts, n_cells, n_unknown)).astype(np.int32)


def free_weights(labels: np.ndarray, n_known: int, n_unknown: int, mask: Optional[np.ndarray] = None) -> np.ndarray:
    """w[B][R * M] float64 of the first windowed M-step: 1 at column r * M + m for a barcode of label Vk + m in restart r; barcodes on a
    known donor, with label -1 or outside the mask get no weight."""
    lab = np.asarray(labels)
    free = np.where(lab >= n_known, lab - n_known, -1)
    return cluster.one_hot_weights(free, n_unknown, mask)


def final_columns(gp: np.ndarray, n_known: int, n_unknown: int, restart: int) -> np.ndarray:
    """[S][Vk + M][3]: the known columns and restart `restart`'s M free columns of an engine's [S][Vk + R M][3] matrix."""
    lo = n_known + restart * n_unknown
    return np.ascontiguousarray(np.concatenate([gp[:, :n_known], gp[:, lo:lo + n_unknown]], axis=1))


def refine_prior(g_known: np.ndarray, q: np.ndarray, n_unknown: int) -> np.ndarray:
    """[S][Vk + M][3] float32: the rounds' prior, the known rows beside q for every unknown column."""
    S = q.shape[0]
    return np.ascontiguousarray(np.concatenate([np.asarray(g_known, dtype=np.float32), np.broadcast_to(q[:, None, :], (S, n_unknown, 3))],
                                               axis=1), dtype=np.float32)


def unknown_calls(assign: np.ndarray, n_known: int) -> np.ndarray:
    """called[b] = m for a barcode called SNG-UNKm (assign = Vk + m), -1 otherwise."""
    a = np.asarray(assign)
    return np.where(a >= n_known, a - n_known, -1)


def write_clust_tsv(path: str, snps, n_known: int, n_unknown: int, ll: np.ndarray, n_cell: np.ndarray, n_ref: np.ndarray, n_alt: np.ndarray,
                    gp: np.ndarray) -> None:
    """<prefix>.clust.tsv: the UNK columns' refined rows (refine.write_refined_tsv's format)."""
    sl = slice(n_known, n_known + n_unknown)
    refine.write_refined_tsv(path, snps, unknown_ids(n_unknown), ll[:, sl], n_cell[:, sl], n_ref[:, sl], n_alt[:, sl], gp[:, sl])


def write_match_tsv(path: str, n_cell: np.ndarray, sum_llk: np.ndarray, known_ids: Sequence[str]) -> None:
    """<prefix>.match.tsv: cluster.write_match_tsv's rows for the UNK columns against every known sample."""
    cluster.write_match_tsv(path, n_cell, sum_llk, known_ids, names=unknown_ids(sum_llk.shape[0]))


def em_loop(eng, pl, S: int, R: int, Vk: int, M: int, q: np.ndarray, floor: float, log_pi: np.ndarray, mask, max_iter: int, tol: float,
            temperature: float, em_rows: Optional[list] = None):
    """The EM iterations after a first windowed M-step (module docstring): returns (ll[R] of the last E-step, log_pi after it,
    iterations).  The engine ends with the M-step of the last E-step's weights."""
    dense = pl.pair_snp is None
    prev = None
    it = 0
    ll = None
    for it in range(1, max_iter + 1):
        eng.set_genotypes_device(eng.cluster_device_ptr(), S)
        if dense:
            eng.set_pileup(pl)          # a dense pileup's SNP-minor copy of the matrix is made when it is staged
        eng.run_singlet()
        ll, cs = eng.cluster_estep_known(R, Vk, M, log_pi, temperature, mask)
        if em_rows is not None:
            em_rows += [(it, r, float(ll[r]), np.exp(log_pi[r])) for r in range(R)]
        log_pi = cluster.update_log_pi(cs, R, Vk + M)
        eng.cluster_mstep_window(None, R, M, q, floor, fetch=False)
        if cluster.converged(prev, ll, tol):
            break
        prev = ll
    return ll, log_pi, it


def partial_run(store_or_pileup, g_known: np.ndarray, known_ids: Sequence[str], n_unknown: int, out_prefix: str, restarts: int = 16,
                seed: int = 0, max_iter: int = 50, tol: float = 1e-7, floor: float = 1e-3, min_snp: int = 0,
                alphas: Sequence[float] = (0.0, 0.5), rounds: int = 1, init_labels: Optional[np.ndarray] = None, match: bool = False,
                barcodes: Optional[Sequence[str]] = None, device: int = 0, mode: int = capi.DMX_MODE_STRICT, doublet_prior: float = 0.5,
                temperature: float = 1.0, snps=None, em_doublets: bool = False, split_merge: bool = False, n_gpus: int = 1) -> dict:
    """Demultiplexes a pool of len(known_ids) genotyped donors (g_known [S][Vk][3]) and n_unknown donors without genotypes (module
    docstring).  `init_labels` ([R][B] int, values in [-1, Vk + M)) replaces the seeded start; its R replaces `restarts`.  With match
    every UNK column's singlets are scored against every known sample (<prefix>.match.tsv): an UNK that best matches a known donor
    flags an n_unknown that is too large.  Doublet components (em_doublets), split-merge moves and several GPUs are not supported.
    Returns a dict: the winning restart, per-restart LL, iterations, the final matrix g[S][Vk + M][3], the prior q[S][3], the sample ids
    and the last round's prefix."""
    if em_doublets or split_merge:
        raise ValueError("partial_run: doublet components (--em-doublets) and split-merge moves (--split-merge) are not supported with "
                         "known donors; use demuxlet_amd.cluster for them")
    if n_gpus != 1:
        raise ValueError(f"partial_run: runs on one GPU, not {n_gpus}")
    if not isinstance(n_unknown, (int, np.integer)):
        raise ValueError(f"n_unknown must be an integer, not {n_unknown!r}: M is not chosen automatically")
    if isinstance(store_or_pileup, engine.HostPileup):
        pl = store_or_pileup
        if barcodes is None:
            raise ValueError("partial_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    g_known = np.ascontiguousarray(g_known, dtype=np.float32)
    B, S, M, R = pl.n_cells, pl.n_snps, int(n_unknown), int(restarts)
    if g_known.ndim != 3 or g_known.shape[0] != S or g_known.shape[2] != 3:
        raise ValueError(f"g_known must be [{S}][Vk][3], not {g_known.shape}")
    Vk = g_known.shape[1]
    known_ids = list(known_ids)
    if init_labels is not None:
        init_labels = check_init_labels(init_labels, B, Vk, M)
        R = init_labels.shape[0]
    check_args(Vk, M, R, known_ids, max_iter, tol, floor, B, len(pl.pair_nrd))
    K, V = Vk + M, Vk + R * M
    mask = pl.n_snp_per_cell >= min_snp if min_snp > 0 else None
    kw = dict(barcodes=barcodes, doublet_prior=doublet_prior, device=device, mode=mode, min_snp=min_snp)
    dense = pl.pair_snp is None
    eng = engine.Engine(V, alphas, doublet_prior, device=device, mode=mode)
    em_rows: list = []
    try:
        # prior: pooled REF / ALT counts of every barcode (one refinement with all barcodes in column 0), as in cluster_run
        flat = np.full((S, V, 3), 1.0 / 3.0, dtype=np.float32)
        eng.set_genotypes(flat)
        eng.set_pileup(pl)
        _, _, n_ref, n_alt, _ = eng.refine_genotypes(np.zeros(B, dtype=np.int32), flat, floor)
        del flat
        q = cluster.hwe_prior(n_ref[:, 0], n_alt[:, 0])
        eng.cluster_stage()
        if init_labels is None:
            # K1 once over [known | q ...]: the known donors' llks and the llk against q (every free column holds q)
            eng.set_genotypes(np.concatenate([g_known, np.broadcast_to(q[:, None, :], (S, R * M, 3))], axis=1))
            if dense:
                eng.set_pileup(pl)
            eng.run_singlet()
            llks, _ = eng.get_singlet()
            labels = initial_labels(llks[:, :Vk], llks[:, Vk], seed, R, M)
            del llks
        else:
            labels = init_labels
        eng.cluster_set_known(g_known)
        eng.cluster_mstep_window(free_weights(labels, Vk, M, mask), R, M, q, floor, fetch=False)
        log_pi = np.full((R, K), -np.log(K))
        ll, log_pi, it = em_loop(eng, pl, S, R, Vk, M, q, floor, log_pi, mask, max_iter, tol, temperature, em_rows)
        win = cluster.best_restart(ll)
        _, _, gp = eng.get_cluster(S)
        g = final_columns(gp, Vk, M, win)
    finally:
        eng.close()
    cluster.write_em_tsv(out_prefix + ".em.tsv", em_rows)
    ids = known_ids + unknown_ids(M)
    engine.demuxlet_run(pl, g, ids, alphas, out_prefix, **kw)
    # rounds: every column refined from the previous round's singlets; the known columns against their VCF rows, the unknown against q
    prior = refine_prior(g_known, q, M)
    reng = engine.Engine(K, alphas, doublet_prior, device=device, mode=mode)
    try:
        reng.set_genotypes(prior)
        reng.set_pileup(pl)
        prev_prefix = out_prefix
        for r in range(1, max(rounds, 1) + 1):
            assign = refine.assignments_from_best(prev_prefix + ".best", ids, barcodes)
            ll_r, n_cell, n_ref_r, n_alt_r, gr = reng.refine_genotypes(assign, prior, floor)
            if r > rounds:
                break                       # rounds = 0: the refinement only feeds <prefix>.clust.tsv
            prev_prefix = f"{out_prefix}.r{r}"
            engine.demuxlet_run(pl, gr, ids, alphas, prev_prefix, **kw)
    finally:
        reng.close()
    write_clust_tsv(out_prefix + ".clust.tsv", snps, Vk, M, ll_r, n_cell, n_ref_r, n_alt_r, gr)
    if match:
        meng = engine.Engine(Vk, alphas, doublet_prior, device=device, mode=mode)
        try:
            meng.set_genotypes(g_known)
            meng.set_pileup(pl)
            meng.run_singlet()
            llks, _ = meng.get_singlet()
        finally:
            meng.close()
        called = unknown_calls(refine.assignments_from_best(prev_prefix + ".best", ids, barcodes), Vk)
        n_cell_m, sum_llk = cluster.match_table(llks, called, M)
        write_match_tsv(out_prefix + ".match.tsv", n_cell_m, sum_llk, known_ids)
    return dict(restart=win, ll=ll, iterations=it, gp=g, prior=q, sample_ids=ids, last_prefix=prev_prefix)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.partial",
                                 description="demultiplexing of a pool whose VCF holds only some of its donors")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`; its samples are the known donors")
    ap.add_argument("--n-unknown", type=int, required=True, help="M, the number of donors in the pool without genotypes")
    ap.add_argument("--out", required=True, help="output prefix: <out>.best/.single/.sing2, <out>.r<N>.*, <out>.em.tsv, <out>.clust.tsv")
    ap.add_argument("--restarts", type=int, default=16, help="independent starts of the unknown donors; the best log-likelihood wins (default 16)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--tol", type=float, default=1e-7, help="stop when every restart's |dLL| < tol * |LL| (default 1e-7)")
    ap.add_argument("--floor", type=float, default=1e-3, help="added to the prior of every covered row (default 1e-3)")
    ap.add_argument("--min-snp", type=int, default=0, help="barcodes with fewer covered SNPs take no part in the EM and get no call")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="grid of alpha values (default 0 0.5)")
    ap.add_argument("--doublet-prior", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=1, help="refinement rounds after the final pass (default 1)")
    ap.add_argument("--match", action="store_true", help="score the unknown donors against the known samples (<out>.match.tsv)")
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST for every pass")
    ap.add_argument("--gpu", type=int, default=0)
    # options of demuxlet_amd.cluster that this mode does not have: named here so that asking for them gives a clear error
    ap.add_argument("--em-doublets", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--split-merge", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.em_doublets or a.split_merge:
        ap.error("--em-doublets and --split-merge are not supported with known donors (use python -m demuxlet_amd.cluster)")
    if a.n_unknown < 1:
        ap.error("--n-unknown must be at least 1")
    if a.restarts < 1:
        ap.error("--restarts must be at least 1")
    return a


def main(argv: Optional[Sequence[str]] = None) -> int:
    a = parse_args(argv)
    d = refine.read_pileup_txt(a.pileup)
    if not d.sample_ids:
        raise SystemExit(f"{a.pileup} has no genotyped samples: a pool without known donors is demultiplexed by python -m demuxlet_amd.cluster")
    partial_run(d.pileup, d.g, d.sample_ids, a.n_unknown, a.out, restarts=a.restarts, seed=a.seed, max_iter=a.max_iter, tol=a.tol,
                floor=a.floor, min_snp=a.min_snp, alphas=a.alpha, rounds=a.rounds, match=a.match, barcodes=d.barcodes, device=a.gpu,
                mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT, doublet_prior=a.doublet_prior, snps=d.snps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
