"""GPU (-m gpu): the `demuxlet` binary end to end — SAM/BAM + VCF in, the four files out — against the oracle run on the
events of the independent scan restatement (tests/sam_vcf_synth.py)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sam_vcf_synth as sv

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "demuxlet_amd" / "demuxlet"
CONTIGS = [("1", 30000), ("2", 20000), ("X", 15000)]
SAMPLES = ["smC", "smA", "smB", "smD"]


def compare_files(got_path, want_path, best=False):
    got = Path(got_path).read_text().splitlines()
    want = Path(want_path).read_text().splitlines()
    assert len(got) == len(want) and got[0] == want[0]
    for a, b in zip(got[1:], want[1:]):
        fa, fb = a.split("\t"), b.split("\t")
        assert len(fa) == len(fb)
        for x, y in zip(fa, fb):
            try:
                fx, fy = float(x), float(y)
                assert abs(fx - fy) <= 1e-3 * max(1e-3, abs(fy)) + 1.01e-4, (a, b)
            except ValueError:
                assert x == y, (a, b)


@pytest.mark.parametrize("field,fmt,extra", [("GT", "bam", ["--write-pair"]), ("GP", "sam", ["--alpha", "0", "--alpha", "0.25", "--alpha", "0.5"]),
                                              ("PL", "sam", ["--min-snp", "5", "--doublet-prior", "0.3"]),
                                              ("PL", "bam", ["--write-pair", "--gpus", "3"]),        # three engines (one device here)
                                              ("PL", "sam", ["--write-pair", "--fast", "--gpus", "2"]),    # DMX_MODE_FAST (opt-in)
                                              ("GT", "sam", ["--fast"]), ("GP", "bam", ["--fast"]),
                                              ("GP", "sam", ["--alpha", "0", "--alpha", "0.25", "--alpha", "0.5", "--fast"]),   # k_doublet_anf
                                              ("PL", "bam", ["--alpha", "0", "--alpha", "0.3", "--fast", "--write-pair"]),
                                              ("GT", "sam", ["--strict"]),                                  # the default (DMX_MODE_STRICT), spelled out
                                              # SAM qualities over 0..93, none skipped or capped: reads beyond the engine's pair / triple / LDS tables
                                              ("GT", "sam", ["--min-BQ", "0", "--cap-BQ", "93", "--write-pair"]),
                                              ("GP", "bam", ["--min-BQ", "0", "--cap-BQ", "93", "--fast"])])
def test_cli_end_to_end(oracle, tmp_path, field, fmt, extra):
    from demuxlet_amd import build
    build.build()
    rng = np.random.default_rng(77 + len(field) + len(extra))
    recs = sv.make_vcf(rng, CONTIGS, 150, SAMPLES, tmp_path / "v.vcf.gz", with_noise=(field != "GP"))
    min_bq = int(extra[extra.index("--min-BQ") + 1]) if "--min-BQ" in extra else 13
    cap_bq = int(extra[extra.index("--cap-BQ") + 1]) if "--cap-BQ" in extra else 40
    reads = sv.make_reads(rng, CONTIGS, recs, 6000, [f"BC{i:02d}-1" for i in range(20)], tmp_path / "r.sam", tmp_path / "r.bam",
                          qual_range=(0, cap_bq + 1) if cap_bq > 41 else (2, 42))
    out = tmp_path / "o"
    subprocess.run([str(CLI), "--sam", str(tmp_path / f"r.{fmt}"), "--vcf", str(tmp_path / "v.vcf.gz"), "--field", field, "--out", str(out)] + extra,
                   check=True, stderr=subprocess.DEVNULL)
    # expectation: scan restatement -> oracle
    snps, events, gts, sm_cols = sv.scan(reads, recs, CONTIGS, SAMPLES, min_bq=min_bq, cap_bq=cap_bq)
    if cap_bq > 41:
        bq = np.array([e[4] for e in events])
        assert bq.min() == 0 and bq.max() == cap_bq
    if field == "GT":
        g = np.stack([oracle.geno_from_gt(np.array(a), 0.01) for a in gts])
    elif field == "PL":
        g = np.stack([oracle.geno_from_pl(np.array([[(np.iinfo(np.int32).min if x == "." else int(x)) for x in (recs[i]["fields"][c].split(":")[1].split(",") + ["."] * 3)[:3]]
                                                    for c in sm_cols])) for i in snps])
    else:
        g = np.stack([oracle.geno_from_gp(np.array([[(np.nan if x == "." else float(x)) for x in (recs[i]["fields"][c].split(":")[2].split(",") + ["."] * 3)[:3]]
                                                    for c in sm_cols], dtype=np.float32), 0.01) for i in snps])
    ev = oracle.Events([e[0] for e in events], np.array([e[1] for e in events], dtype=np.int32), [e[2] for e in events],
                       np.array([e[3] for e in events], dtype=np.uint8), np.array([e[4] for e in events], dtype=np.uint8),
                       np.array([e[5] for e in events], dtype=np.uint8))
    alphas = tuple(float(extra[i + 1]) for i, x in enumerate(extra) if x == "--alpha") or (0.0, 0.5)
    params = oracle.Params(alphas=alphas, write_pair="--write-pair" in extra,
                           min_snp=int(extra[extra.index("--min-snp") + 1]) if "--min-snp" in extra else 0,
                           doublet_prior=float(extra[extra.index("--doublet-prior") + 1]) if "--doublet-prior" in extra else 0.5)
    pb = oracle.Problem(SAMPLES, np.nan_to_num(g.astype(np.float32)), ev, params)
    oracle.run_problem(pb, str(tmp_path / "orc"))
    for suf in ["single", "sing2", "best"] + (["pair"] if "--write-pair" in extra else []):
        compare_files(f"{out}.{suf}", tmp_path / f"orc.{suf}")
    got_best = [l.split("\t")[5] for l in Path(f"{out}.best").read_text().splitlines()]
    want_best = [l.split("\t")[5] for l in (tmp_path / "orc.best").read_text().splitlines()]
    assert got_best == want_best


def test_nan_likelihoods_do_not_crash(tmp_path):
    """A GP record with a missing sample turns the whole SNP into NaN (bcf_filtered_reader.cpp:431-448) and the reference then
    indexes its grid with -1; the product must neither fault on the GPU nor on the host, and must still write all files."""
    from demuxlet_amd import build
    build.build()
    rng = np.random.default_rng(3)
    recs = sv.make_vcf(rng, CONTIGS, 100, SAMPLES, tmp_path / "v.vcf.gz", with_noise=True)
    sv.make_reads(rng, CONTIGS, recs, 3000, [f"BC{i:02d}-1" for i in range(10)], tmp_path / "r.sam")
    r = subprocess.run([str(CLI), "--sam", str(tmp_path / "r.sam"), "--vcf", str(tmp_path / "v.vcf.gz"), "--field", "GP", "--out", str(tmp_path / "o"),
                        "--write-pair"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-500:]
    for suf in ("single", "sing2", "best", "pair"):
        assert (tmp_path / f"o.{suf}").stat().st_size > 100
    # the hot path's own notices (cmd_cram_demuxlet.cpp:406,:468,:524,:876), in the reference's order, with its droplet count
    n_drop = (len((tmp_path / "o.single").read_text().splitlines()) - 1) // len(SAMPLES)
    msgs = [ln.split("] - ", 1)[1] for ln in r.stderr.splitlines() if ln.startswith("NOTICE")]
    tail = [m for m in msgs if m.startswith(("Starting to identify", "Identifying best", "Finished processing", "Finished writing"))]
    assert tail == ["Starting to identify best matching individual IDs", "Identifying best-matching individual..",
                    f"Finished processing {n_drop} droplets total", "Finished writing output files"], tail


def test_cfg1_tutorial_vcf_through_the_binary_on_the_gpu(oracle, tmp_path):
    """BASELINE config 1 on the HIP path: the reference tutorial's VCF (tutorial/README.MD; first 4 000 records, a data fixture —
    the tutorial BAM is not in the reference repository) + a synthetic 500-barcode SAM laid over it, `--field GT --alpha 0
    --alpha 0.5` through the `demuxlet` binary on the GPU, against the oracle's four files for the same scan."""
    import gzip
    from demuxlet_amd import build
    build.build()
    vcf = ROOT / "tests" / "golden" / "tutorial_jurkat_293T_first4000.vcf.gz"
    recs, contigs = [], []
    for line in gzip.open(vcf, "rt"):
        if line.startswith("##contig=<ID="):
            name = line[13:].split(",")[0].rstrip(">\n")
            ln = int(line.split("length=")[1].split(">")[0].split(",")[0]) if "length=" in line else 250000000
            contigs.append((name, ln))
        elif not line.startswith("#"):
            t = line.rstrip("\n").split("\t")
            recs.append(dict(chrom=t[0], pos=int(t[1]) - 1, ref=t[3], alt=t[4], fields=t[9:]))
    rng = np.random.default_rng(20)
    used = [c for c in contigs if c[0] in {r["chrom"] for r in recs}]
    samples = ["jurkat", "293T_RTG"]
    reads = sv.make_reads(rng, used, recs, 40000, [f"CELL{i:03d}-1" for i in range(500)], tmp_path / "r.sam", tmp_path / "r.bam")
    out = tmp_path / "o"
    subprocess.run([str(CLI), "--sam", str(tmp_path / "r.bam"), "--vcf", str(vcf), "--field", "GT", "--alpha", "0", "--alpha", "0.5",
                    "--out", str(out)], check=True, stderr=subprocess.DEVNULL)
    snps, events, gts, sm_cols = sv.scan(reads, recs, used, samples)
    assert len(snps) > 500
    g = np.stack([oracle.geno_from_gt(np.array(a), 0.01) for a in gts])
    ev = oracle.Events([e[0] for e in events], np.array([e[1] for e in events], dtype=np.int32), [e[2] for e in events],
                       np.array([e[3] for e in events], dtype=np.uint8), np.array([e[4] for e in events], dtype=np.uint8),
                       np.array([e[5] for e in events], dtype=np.uint8))
    oracle.run_problem(oracle.Problem(samples, g.astype(np.float32), ev, oracle.Params()), str(tmp_path / "orc"))
    for suf in ("single", "sing2", "best"):
        compare_files(f"{out}.{suf}", tmp_path / f"orc.{suf}")
    got = [l.split("\t") for l in Path(f"{out}.best").read_text().splitlines()]
    want = [l.split("\t") for l in (tmp_path / "orc.best").read_text().splitlines()]
    assert len(got) > 300 and [r[5] for r in got] == [r[5] for r in want]         # every BEST call
    assert [r[:5] for r in got] == [r[:5] for r in want]                            # barcodes and read/SNP counters
    calls = {r[5][:3] for r in got[1:]}
    assert "SNG" in calls                                                          # the job is not degenerate
    # the same genotypes as BCF2: the same three files, byte for byte
    sv.vcf_text_to_bcf(gzip.open(vcf, "rt").read(), tmp_path / "t.bcf")
    outb = tmp_path / "ob"
    subprocess.run([str(CLI), "--sam", str(tmp_path / "r.bam"), "--vcf", str(tmp_path / "t.bcf"), "--field", "GT", "--alpha", "0", "--alpha", "0.5",
                    "--out", str(outb)], check=True, stderr=subprocess.DEVNULL)
    for suf in ("single", "sing2", "best"):
        assert Path(f"{outb}.{suf}").read_bytes() == Path(f"{out}.{suf}").read_bytes(), suf


def _tutorial_records(vcf):
    import gzip
    recs, contigs, fmt = [], [], None
    for line in gzip.open(vcf, "rt"):
        if line.startswith("##contig=<ID="):
            name = line[13:].split(",")[0].rstrip(">\n")
            ln = int(line.split("length=")[1].split(">")[0].split(",")[0]) if "length=" in line else 250000000
            contigs.append((name, ln))
        elif not line.startswith("#"):
            t = line.rstrip("\n").split("\t")
            recs.append(dict(chrom=t[0], pos=int(t[1]) - 1, ref=t[3], alt=t[4], fields=t[9:], fmt=t[8].split(":")))
    return recs, contigs


def test_cfg1_at_size_full_tutorial_vcf(oracle, tmp_path):
    """BASELINE config 1 at its size: ALL 54 424 records of the reference tutorial's VCF (tutorial/README.MD:56-61;
    shipped as a data fixture — the tutorial BAM is not in the reference repository) against a synthetic 500-barcode BAM laid over
    all of its 24 contigs, through the `demuxlet` binary on the GPU, `--field GT` (the tutorial's command line: default alphas {0, 0.5},
    cmd_cram_demuxlet.cpp:78-90) and `--field PL` (the file's real PL values through the 10-iteration EM, bcf_filtered_reader.cpp:244-320),
    against the oracle run on the independent scan restatement.  More than 20 000 of the records that pass the variant filter have
    a missing second sample and take the Hardy-Weinberg fallback of bcf_filtered_reader.cpp:381-388 (GT) or enter the EM with all
    three likelihoods at the clamp (PL)."""
    from demuxlet_amd import build
    build.build()
    vcf = ROOT / "tests" / "golden" / "tutorial_jurkat_293T_exons_only.vcf.gz"
    recs, contigs = _tutorial_records(vcf)
    assert len(recs) == 54424
    rng = np.random.default_rng(2024)
    used = [c for c in contigs if c[0] in {r["chrom"] for r in recs}]
    assert len(used) == 24
    samples = ["jurkat", "293T_RTG"]
    reads = sv.make_reads(rng, used, recs, 150000, [f"CELL{i:03d}-1" for i in range(500)], tmp_path / "r.sam", tmp_path / "r.bam")
    snps, events, gts, sm_cols = sv.scan(reads, recs, used, samples)
    n_missing = sum(1 for a in gts if any(x < 0 for x in a[1]))
    print(f"cfg1 at size: {len(recs)} VCF records, {len(snps)} pass the variant filter and enter the scan, {n_missing} of them with a missing 293T_RTG "
          f"genotype (HWE fallback); {len(events)} scan events from {len(reads)} reads")
    assert len(snps) > 25000 and n_missing > 20000
    ev = oracle.Events([e[0] for e in events], np.array([e[1] for e in events], dtype=np.int32), [e[2] for e in events],
                       np.array([e[3] for e in events], dtype=np.uint8), np.array([e[4] for e in events], dtype=np.uint8),
                       np.array([e[5] for e in events], dtype=np.uint8))
    g_gt = np.stack([oracle.geno_from_gt(np.array(a), 0.01) for a in gts]).astype(np.float32)
    # the HWE rows really are in the matrix: a missing sample's GT row is the smoothed Hardy-Weinberg vector, a called one the 0.99 one-hot
    missing = np.array([[any(x < 0 for x in smp) for smp in a] for a in gts])
    assert missing.sum() > 25000 and (g_gt[missing].max(axis=1) < 0.98).all() and (g_gt[~missing].max(axis=1) > 0.98).all()

    def run_and_compare(tag, vcf_path, field, g, ev, extra):
        out = tmp_path / f"o_{tag}"
        subprocess.run([str(CLI), "--sam", str(tmp_path / "r.bam"), "--vcf", str(vcf_path), "--field", field, "--out", str(out)] + extra,
                       check=True, stderr=subprocess.DEVNULL)
        wp = "--write-pair" in extra
        oracle.run_problem(oracle.Problem(samples, g, ev, oracle.Params(write_pair=wp)), str(tmp_path / f"orc_{tag}"))
        for suf in ("single", "sing2", "best") + (("pair",) if wp else ()):
            if "--fast" in extra:
                compare_files(f"{out}.{suf}", tmp_path / f"orc_{tag}.{suf}")
            else:                                                       # STRICT (the default): the oracle's bytes
                assert Path(f"{out}.{suf}").read_bytes() == (tmp_path / f"orc_{tag}.{suf}").read_bytes(), (tag, suf)
        got = [l.split("\t") for l in Path(f"{out}.best").read_text().splitlines()]
        want = [l.split("\t") for l in (tmp_path / f"orc_{tag}.best").read_text().splitlines()]
        assert len(got) > 400 and [r[:6] for r in got] == [r[:6] for r in want]
        assert {"SNG"} <= {r[5][:3] for r in got[1:]}

    run_and_compare("gt", vcf, "GT", g_gt, ev, [])                                                   # the tutorial's command line
    run_and_compare("gtx", vcf, "GT", g_gt, ev, ["--alpha", "0", "--alpha", "0.5", "--write-pair"])  # README.md:12's advice, spelled out
    run_and_compare("gtf", vcf, "GT", g_gt, ev, ["--fast"])

    # --field PL on the file as it is: 16 584 of its records carry no PL (FORMAT GT:RE:GQ:DP:RS), and the reference stops at the first
    # one the scan reaches (bcf_get_format_int32 < 0 -> parse_likelihoods false -> error(), cmd_cram_demuxlet.cpp:211-212).  Same here.
    first_without = next(r for r in recs if "PL" not in r["fmt"])
    r = subprocess.run([str(CLI), "--sam", str(tmp_path / "r.bam"), "--vcf", str(vcf), "--field", "PL", "--out", str(tmp_path / "plfull")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and f"Cannot parse posterior probability at {first_without['chrom']}:{first_without['pos'] + 1}" in r.stderr

    # the 37 840 records that do carry PL, with the file's real values (PL of a missing sample: '.', all three likelihoods at the clamp)
    import gzip
    keep = [l for l in gzip.open(vcf, "rt") if l.startswith("#") or "PL" in l.split("\t")[8].split(":")]
    with gzip.open(tmp_path / "pl.vcf.gz", "wt") as f:
        f.writelines(keep)
    recs_pl = [r for r in recs if "PL" in r["fmt"]]
    assert len(recs_pl) == 25259 + 12581
    snps2, events2, gts2, sm2 = sv.scan(reads, recs_pl, used, samples)
    ev2 = oracle.Events([e[0] for e in events2], np.array([e[1] for e in events2], dtype=np.int32), [e[2] for e in events2],
                        np.array([e[3] for e in events2], dtype=np.uint8), np.array([e[4] for e in events2], dtype=np.uint8),
                        np.array([e[5] for e in events2], dtype=np.uint8))
    imin = np.iinfo(np.int32).min

    def pl_of(rec, c):
        f = rec["fields"][c].split(":")
        k = rec["fmt"].index("PL")
        v = f[k].split(",") if k < len(f) else ["."]
        return [(imin if x == "." else int(x)) for x in (v + ["."] * 3)[:3]]

    g_pl = np.stack([oracle.geno_from_pl(np.array([pl_of(recs_pl[i], c) for c in sm2])) for i in snps2]).astype(np.float32)
    n_missing_pl = sum(1 for i in snps2 if recs_pl[i]["fields"][1].split(":")[0] == ".")
    print(f"   PL subset: {len(recs_pl)} records, {len(snps2)} enter the scan, {n_missing_pl} with a missing second sample")
    assert n_missing_pl > 20000
    run_and_compare("pl", tmp_path / "pl.vcf.gz", "PL", g_pl, ev2, [])
    run_and_compare("plf", tmp_path / "pl.vcf.gz", "PL", g_pl, ev2, ["--fast", "--gpus", "2"])
    # a lone `--alpha 0.5` (BASELINE.json's wording) leaves the reference with nAlpha = 1: its doublet scan (:799-814, n from 1) finds
    # nothing and :820-826 index the grid with -1 — undefined behaviour.  The binary refuses instead of inventing an answer.
    r = subprocess.run([str(CLI), "--sam", str(tmp_path / "r.bam"), "--vcf", str(vcf), "--field", "GT", "--alpha", "0.5", "--out", str(tmp_path / "lone")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and ">= 2 alphas" in r.stderr
