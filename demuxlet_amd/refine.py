"""Genotype refinement from called singlets, and the iterated demultiplexing pass built on it.

After one demultiplexing pass, the reads of every confidently called singlet are direct evidence of that sample's genotype.  The engine
pools them per (SNP, sample) on the GPU (Engine.refine_genotypes, dmx_engine_refine_genotypes): the summed log
genotype likelihoods, the cell / REF / ALT read counts, and a posterior gp' = prior x likelihood that replaces soft or wrong VCF rows.
`refine_run` iterates: round 0 is the plain `demuxlet_run`, round r >= 1 takes the singlets of round r - 1's `.best`, refines the
original matrix with them and runs again with the refined one.

    python -m demuxlet_amd.refine --pileup <x>.pileup.txt --out <prefix> [--rounds N] [--alpha A ...] [--floor F] [--fast]

reads the dump that `demuxlet --pileup-only` writes (sample ids, SNP records, the genotype matrix in hex floats, cells, pairs with reads)."""
from __future__ import annotations

import argparse
import sys
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import capi, engine

REFINED_HEADER = "RID\tPOS\tREF\tALT\tSM_ID\tN.CELL\tN.REF\tN.ALT\tLLK0\tLLK1\tLLK2\tGP0\tGP1\tGP2\n"


@dataclass
class PileupDump:
    """What `demuxlet --pileup-only` writes to <out>.pileup.txt."""
    sample_ids: List[str]
    snps: List[Tuple[int, int, str, str]]      # (rid, pos, ref, alt) per SNP id
    g: np.ndarray                              # float32 [S][V][3]
    barcodes: List[str]                        # by cell id
    pileup: engine.HostPileup                  # sparse layout (pair_snp present)


def read_pileup_txt(path: str) -> PileupDump:
    nv = ns = nc = 0
    sample_ids: List[str] = []
    snps: List[Tuple[int, int, str, str]] = []
    grows: List[List[float]] = []
    barcodes: List[str] = []
    totl: List[int] = []; pas: List[int] = []; uniq: List[int] = []
    pair_off = [0]; read_off = [0]
    pair_snp: List[int] = []; pair_nrd: List[int] = []; reads = bytearray()
    with open(path) as f:
        for line in f:
            t = line.rstrip("\n").split("\t")
            tag = t[0]
            if tag == "PAIR":
                if not barcodes:
                    raise ValueError(f"{path}: PAIR row before the first CELL row")
                n = int(t[2])
                if len(t) != 3 + n:
                    raise ValueError(f"{path}: PAIR row with {len(t) - 3} reads, count {n}")
                pair_snp.append(int(t[1])); pair_nrd.append(n)
                for r in t[3:]:
                    a, q = r.split(":")
                    reads.append((int(a) << 7) | int(q))
                pair_off[-1] += 1; read_off[-1] += n
            elif tag == "CELL":
                if int(t[1]) != len(barcodes):
                    raise ValueError(f"{path}: cell {t[1]} out of order")
                pair_off.append(pair_off[-1]); read_off.append(read_off[-1])     # the new cell's end, grown by its PAIR rows
                barcodes.append(t[2]); totl.append(int(t[3])); pas.append(int(t[4])); uniq.append(int(t[5]))
            elif tag == "SNP":
                if int(t[1]) != len(snps):
                    raise ValueError(f"{path}: SNP {t[1]} out of order")
                snps.append((int(t[2]), int(t[3]), t[4], t[5]))
                grows.append([float.fromhex(x) for x in t[6:]])
            elif tag == "SM":
                sample_ids.append(t[1])
            elif tag == "NV":
                nv = int(t[1])
            elif tag == "NSNP":
                ns = int(t[1])
            elif tag == "NCELL":
                nc = int(t[1])
            elif tag:
                raise ValueError(f"{path}: unknown row {tag!r}")
    if len(sample_ids) != nv or len(snps) != ns or len(barcodes) != nc:
        raise ValueError(f"{path}: header says {nv} samples, {ns} SNPs, {nc} cells; found {len(sample_ids)}, {len(snps)}, {len(barcodes)}")
    g = np.array(grows, dtype=np.float64).reshape(ns, nv, 3).astype(np.float32)
    po = np.array(pair_off, dtype=np.int64)       # [0, end of cell 0, end of cell 1, ...]: CSR offsets [B + 1]
    ro = np.array(read_off, dtype=np.int64)
    nrd = np.array(pair_nrd, dtype=np.int64)
    mx = int(nrd.max()) if len(nrd) else 0
    nrd = nrd.astype(np.uint8 if mx <= 0xFF else (np.uint16 if mx <= 0xFFFF else np.uint32))
    pl = engine.HostPileup(nc, ns, po, ro, np.array(pair_snp, dtype=np.int32), nrd, np.frombuffer(bytes(reads), dtype=np.uint8).copy(),
                           np.array(totl, dtype=np.int32), np.array(pas, dtype=np.int32), np.array(uniq, dtype=np.int32))
    return PileupDump(sample_ids, snps, g, barcodes, pl)


def write_pileup_txt(path: str, d: PileupDump) -> None:
    """The dump in `demuxlet --pileup-only`'s row format (hex floats in Python's spelling, which float.fromhex reads like C's %a)."""
    pl = d.pileup
    V, S, B = len(d.sample_ids), len(d.snps), pl.n_cells
    with open(path, "w") as f:
        f.write(f"NV\t{V}\nNSNP\t{S}\nNCELL\t{B}\n")
        for sm in d.sample_ids:
            f.write(f"SM\t{sm}\n")
        for s, (rid, pos, ref, alt) in enumerate(d.snps):
            f.write(f"SNP\t{s}\t{rid}\t{pos}\t{ref}\t{alt}\t" + "\t".join(float(x).hex() for x in d.g[s].reshape(-1)) + "\n")
        for c in range(B):
            f.write(f"CELL\t{c}\t{d.barcodes[c]}\t{int(pl.rd_totl[c])}\t{int(pl.rd_pass[c])}\t{int(pl.rd_uniq[c])}\n")
            r = int(pl.cell_read_off[c])
            for p in range(int(pl.cell_pair_off[c]), int(pl.cell_pair_off[c + 1])):
                snp = int(pl.pair_snp[p]) if pl.pair_snp is not None else p - int(pl.cell_pair_off[c])
                n = int(pl.pair_nrd[p])
                f.write(f"PAIR\t{snp}\t{n}" + "".join(f"\t{int(b) >> 7}:{int(b) & 127}" for b in pl.reads[r:r + n]) + "\n")
                r += n


def assignments_from_best(path: str, sample_ids: Sequence[str], barcodes: Sequence[str], min_prb: float = 0.0) -> np.ndarray:
    """assign[cell id] = sample index of the barcode's singlet call in a `.best` file, -1 elsewhere.  Only rows whose BEST starts with
    `SNG-` count; the sample is read from the SNG.1ST column (sample ids may contain '-'); with min_prb > 0 a row also needs
    PRB.SNG1 >= min_prb (cmd_cram_demuxlet.cpp:571, :845)."""
    smap: Dict[str, int] = {s: j for j, s in enumerate(sample_ids)}
    cmap: Dict[str, int] = {b: c for c, b in enumerate(barcodes)}
    out = np.full(len(barcodes), -1, dtype=np.int32)
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        col = {n: i for i, n in enumerate(head)}
        for n in ("BARCODE", "BEST", "SNG.1ST", "PRB.SNG1"):
            if n not in col:
                raise ValueError(f"{path}: no {n} column")
        for line in f:
            t = line.rstrip("\n").split("\t")
            if len(t) < len(head) or not t[col["BEST"]].startswith("SNG-"):
                continue
            if min_prb > 0.0 and not float(t[col["PRB.SNG1"]]) >= min_prb:
                continue
            c, j = cmap.get(t[col["BARCODE"]]), smap.get(t[col["SNG.1ST"]])
            if c is None or j is None:
                raise ValueError(f"{path}: barcode {t[col['BARCODE']]!r} / sample {t[col['SNG.1ST']]!r} not in this job")
            out[c] = j
    return out


def write_refined_tsv(path: str, snps: Optional[Sequence[Tuple]], sample_ids: Sequence[str], ll: np.ndarray, n_cell: np.ndarray,
                      n_ref: np.ndarray, n_alt: np.ndarray, gp: np.ndarray) -> None:
    """<prefix>.refined.tsv: one row per covered (SNP, sample) — N.CELL > 0 — by SNP, then sample.  Without SNP records (a job built
    from a store) RID / REF / ALT are '.' and POS is the SNP id."""
    with open(path, "w") as f:
        f.write(REFINED_HEADER)
        for i, v in zip(*np.nonzero(n_cell > 0)):
            rid, pos, ref, alt = snps[i] if snps is not None else (".", int(i), ".", ".")
            l, q = ll[i, v], gp[i, v]
            f.write(f"{rid}\t{pos}\t{ref}\t{alt}\t{sample_ids[v]}\t{n_cell[i, v]}\t{n_ref[i, v]}\t{n_alt[i, v]}\t"
                    f"{l[0]:.5f}\t{l[1]:.5f}\t{l[2]:.5f}\t{float(q[0]):.6g}\t{float(q[1]):.6g}\t{float(q[2]):.6g}\n")


def refine_run(store_or_pileup, g: np.ndarray, sample_ids: Sequence[str], alphas: Sequence[float], out_prefix: str, rounds: int = 1,
               floor: float = 1e-3, min_prb: float = 0.0, snps: Optional[Sequence[Tuple]] = None, **demuxlet_run_kwargs):
    """Round 0: demuxlet_run(store_or_pileup, g, ...) to out_prefix, unchanged (rounds = 0 is exactly a plain run).  Round r >= 1: the
    singlets of the previous round's .best refine the ORIGINAL matrix g (the prior of every round: the reads are counted once), and
    demuxlet_run goes again with the refined matrix to f"{out_prefix}.r{r}".  The last round's refinement goes to
    <out_prefix>.refined.tsv.  `store_or_pileup` is a Store, or a HostPileup with barcodes=... as for demuxlet_run.
    Returns the refined matrix of the last round (g itself when rounds = 0)."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    engine.demuxlet_run(store_or_pileup, g, sample_ids, alphas, out_prefix, **demuxlet_run_kwargs)
    if rounds <= 0:
        return g
    if isinstance(store_or_pileup, engine.HostPileup):
        pl, barcodes = store_or_pileup, demuxlet_run_kwargs.get("barcodes")
        if barcodes is None:
            raise ValueError("refine_run: a HostPileup needs barcodes=")
    else:
        pl, barcodes = store_or_pileup.freeze(), store_or_pileup.barcodes()
    kw = dict(demuxlet_run_kwargs)
    kw["barcodes"] = barcodes
    eng = engine.Engine(len(sample_ids), alphas, kw.get("doublet_prior", 0.5), device=kw.get("device", 0), mode=kw.get("mode", capi.DMX_MODE_STRICT))
    try:
        eng.set_genotypes(g)
        eng.set_pileup(pl)
        prev, cur = out_prefix, g
        for r in range(1, rounds + 1):
            assign = assignments_from_best(prev + ".best", sample_ids, barcodes, min_prb)
            ll, n_cell, n_ref, n_alt, cur = eng.refine_genotypes(assign, g, floor)
            prev = f"{out_prefix}.r{r}"
            engine.demuxlet_run(pl, cur, sample_ids, alphas, prev, **kw)
        write_refined_tsv(out_prefix + ".refined.tsv", snps, sample_ids, ll, n_cell, n_ref, n_alt, cur)
    finally:
        eng.close()
    return cur


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m demuxlet_amd.refine", description="iterated demultiplexing with genotypes refined from called singlets")
    ap.add_argument("--pileup", required=True, help="<x>.pileup.txt written by `demuxlet --pileup-only`")
    ap.add_argument("--out", required=True, help="output prefix: <out>.best/.single/.sing2 (round 0), <out>.r<N>.* (round N), <out>.refined.tsv")
    ap.add_argument("--rounds", type=int, default=1, help="refinement rounds after the first pass (default 1)")
    ap.add_argument("--alpha", type=float, nargs="+", default=[0.0, 0.5], help="grid of alpha values (default 0 0.5)")
    ap.add_argument("--doublet-prior", type=float, default=0.5)
    ap.add_argument("--floor", type=float, default=1e-3, help="added to every prior entry of a covered row (default 1e-3)")
    ap.add_argument("--min-prb", type=float, default=0.0, help="use only singlets with PRB.SNG1 >= this (default: all SNG- calls)")
    ap.add_argument("--fast", action="store_true", help="DMX_MODE_FAST for every pass")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    d = read_pileup_txt(a.pileup)
    refine_run(d.pileup, d.g, d.sample_ids, a.alpha, a.out, rounds=a.rounds, floor=a.floor, min_prb=a.min_prb, snps=d.snps,
               barcodes=d.barcodes, doublet_prior=a.doublet_prior, device=a.gpu, mode=capi.DMX_MODE_FAST if a.fast else capi.DMX_MODE_STRICT)
    return 0


if __name__ == "__main__":
    sys.exit(main())
