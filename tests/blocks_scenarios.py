"""The three scenarios of the block statistics (test_blocks_cpu.py runs them through the oracle's values, test_gpu_blocks.py through the
kernel): data only — pileups, genotype matrices, truth and the planted block.  8 donors, 1 200 SNPs on one chromosome in 12 blocks of 100,
about 150 covered SNPs per barcode (each SNP covered with probability 0.125), 1 + Poisson(1) reads per pair at base quality 20..40 with
the sequencing error that quality states; 120 singlets (barcode c is donor c mod 8) then 30 doublets (a second donor, half the reads).

  clean   nothing planted.
  soup    barcodes 0..29 (singlets) get another donor's reads in block SOUP_BLOCK only: there every SNP is covered with probability
          SOUP_COVER and a read comes from donor (d + 3) mod 8 with probability SOUP_SHARE.
  swap    the genotype columns of donors SWAP_DONORS are exchanged inside block SWAP_BLOCK only; the reads are the clean pool's.

Each scenario is fixed by its seed; the seeds and the soup's strength were chosen on the CPU, through tests/blocks_ref.py, so that the
reference's values alone meet the outcomes the tests state."""
import numpy as np

V, S, G, B_SNG, B_DBL = 8, 1200, 12, 120, 30
DELTA = 0.125
SEEDS = dict(clean=9101, soup=9102, swap=9113)
SOUP_CELLS, SOUP_BLOCK, SOUP_COVER, SOUP_SHARE = 30, 5, 0.9, 0.7
SWAP_DONORS, SWAP_BLOCK = (2, 5), 7
ALPHAS = (0.0, 0.5)


def block_of_snp():
    return (np.arange(S) // (S // G)).astype(np.int32)


def snp_table():
    return [(1, 1000 * i + 1, "A", "C") for i in range(S)]


def scenario(engine, synth, name):
    """dict(pl = engine.HostPileup, g, truth [B][2] (-1 = no second donor), block [S], barcodes, sample_ids, soup = the soupy barcodes)."""
    rng = np.random.default_rng(SEEDS[name])
    alleles = synth.make_raw_genotypes(rng, S, V).alleles
    dosage = np.clip(alleles, 0, 1).sum(axis=2)
    g = np.stack([engine.geno_from_gt(alleles[s], 0.01) for s in range(S)])
    block = block_of_snp()
    B = B_SNG + B_DBL
    first = np.arange(B) % V
    second = np.where(np.arange(B) >= B_SNG, (first + 1 + rng.integers(0, V - 1, size=B)) % V, -1)
    soup = np.arange(SOUP_CELLS) if name == "soup" else np.zeros(0, dtype=np.int64)
    snps_l, nrd_l, reads_l = [], [], []
    for c in range(B):
        p_cov = np.full(S, DELTA)
        if c in soup:
            p_cov[block == SOUP_BLOCK] = SOUP_COVER
        sn = np.flatnonzero(rng.random(S) < p_cov).astype(np.int32)
        nrd = 1 + rng.poisson(1.0, size=len(sn))
        pr = np.repeat(np.arange(len(sn)), nrd)
        src = np.full(len(pr), first[c])
        if second[c] >= 0:
            src = np.where(rng.random(len(pr)) < 0.5, second[c], first[c])
        if c in soup:
            src = np.where((block[sn[pr]] == SOUP_BLOCK) & (rng.random(len(pr)) < SOUP_SHARE), (first[c] + 3) % V, src)
        alt = rng.random(len(pr)) < dosage[sn[pr], src] / 2.0
        bq = rng.integers(20, 41, size=len(pr))
        alt ^= rng.random(len(pr)) < 10.0 ** (-bq / 10.0)
        snps_l.append(sn); nrd_l.append(nrd.astype(np.uint8)); reads_l.append((bq | (alt.astype(np.int64) << 7)).astype(np.uint8))
    cpo = np.concatenate([[0], np.cumsum([len(x) for x in snps_l])]).astype(np.int64)
    cro = np.concatenate([[0], np.cumsum([len(x) for x in reads_l])]).astype(np.int64)
    tot = np.diff(cro).astype(np.int32)
    pl = engine.HostPileup(B, S, cpo, cro, np.concatenate(snps_l), np.concatenate(nrd_l), np.concatenate(reads_l), tot, tot.copy(), tot.copy())
    if name == "swap":
        a, b = SWAP_DONORS
        rows = block == SWAP_BLOCK
        g = g.copy()
        g[np.ix_(rows, [a, b])] = g[np.ix_(rows, [b, a])]
    return dict(pl=pl, g=g, truth=np.stack([first, second], axis=1).astype(np.int32), block=block, soup=soup,
                barcodes=[synth.barcode_name(c) for c in range(B)], sample_ids=[f"s{j}" for j in range(V)])


def check_outcome(name, sc, kind, sng1, calls, loo_labels, donors):
    """The outcome each scenario states, on the statistics of either suite: kind / sng1 are the `.best` rows' (0 = SNG, 1 = DBL, 2 = AMB),
    calls = blocks.block_calls' dict, loo_labels the LOO.CALL strings, donors = blocks.block_donors' rows.  Returns the figures it saw."""
    truth, flag = sc["truth"], np.asarray(calls["flag"])
    sng, dbl = np.flatnonzero(truth[:, 1] < 0), np.flatnonzero(truth[:, 1] >= 0)
    swap_rows = [(r[0], r[1], r[6]) for r in donors if r[7] == "SWAP?"]
    if name == "clean":
        assert not (flag == "FRAGILE").any(), np.flatnonzero(flag == "FRAGILE")
        assert swap_rows == []
    elif name == "soup":
        soup = sc["soup"]
        mis = soup[kind[soup] == 1]
        assert 2 * len(mis) >= len(soup), f"the plain pass calls only {len(mis)} of {len(soup)} soupy singlets DBL-"
        for b in mis:
            assert flag[b] == "FRAGILE" and calls["top_block"][b] == SOUP_BLOCK and loo_labels[b] == f"SNG-s{truth[b, 0]}", \
                (b, flag[b], calls["top_block"][b], loo_labels[b])
        assert (flag[dbl] == "STABLE").all(), dbl[flag[dbl] != "STABLE"]
        return dict(n_miscalled=len(mis))
    else:
        assert (kind[sng] == 0).all() and (sng1[sng] == truth[sng, 0]).all()
        a, b = SWAP_DONORS
        assert sorted(swap_rows) == [(a, SWAP_BLOCK, b), (b, SWAP_BLOCK, a)], swap_rows
    return dict(n_fragile=int((flag == "FRAGILE").sum()), n_swap=len(swap_rows))
