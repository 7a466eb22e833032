"""The SNP-variant rule (include/nprealign.h: npr_snp_variants_table) on hand-made rows through the numpy restatement of
snp_variants_reference.py, the VCF / FASTQ writers of analyses/consensus.py byte for byte, and the plumbing that needs no GPU."""
import numpy as np

from snp_variants_reference import snp_variants_reference

FLAT = np.where(np.eye(4, dtype=bool), 0.8, 0.2 / 3)


def test_rows_that_cannot_be_called_have_no_base_and_no_call():
    weights = np.array([[9.0, 1.0, 0.0, 0.0],    # never seen (whatever it holds)
                        [0.0, 0.0, 0.0, 0.0],    # seen, nothing counted
                        [9.0, 1.0, 0.0, 0.0],    # the reference base is N
                        [9.0, 1.0, 0.0, 0.0]])   # callable
    got = snp_variants_reference(weights, [0, 1, 1, 1], [0, 1, 4, 2], FLAT, 0.0)
    assert got["callable"].tolist() == [False, False, False, True]
    assert got["best"].tolist() == [4, 4, 4, 0] and got["qual"][:3].tolist() == [0, 0, 0]
    assert got["call_row"].tolist() == [3, 3, 3] and got["call_alt"].tolist() == [0, 1, 3]   # every candidate but the reference's G
    # lp = 0.9 log e[c][A] + 0.1 log e[c][C]: by hand
    lp = np.array([0.9 * np.log(0.8) + 0.1 * np.log(0.2 / 3), 0.9 * np.log(0.2 / 3) + 0.1 * np.log(0.8), np.log(0.2 / 3), np.log(0.2 / 3)])
    p = np.exp(lp) / np.exp(lp).sum()
    assert np.allclose(got["call_p"], p[[0, 1, 3]], rtol=1e-13, atol=0)
    assert got["qual"][3] == int(np.floor(-10 * np.log10(1 - p[0])))


def test_an_impossible_candidate_is_a_call_at_threshold_zero_only():
    evolution = np.array([[1.0, 0.0, 1.0, 1.0]] * 4)   # nothing evolves into C
    weights, seen, ref = [[1.0, 5.0, 1.0, 1.0]], [1], [0]
    at_zero = snp_variants_reference(weights, seen, ref, FLAT, 0.0, evolution)
    assert at_zero["call_alt"].tolist() == [1, 2, 3] and at_zero["call_p"][0] == 0.0 and (at_zero["call_p"][1:] > 0).all()
    assert at_zero["best"][0] != 1
    above = snp_variants_reference(weights, seen, ref, FLAT, 1e-300, evolution)
    assert above["call_alt"].tolist() == [2, 3]


def test_quality_is_capped_at_93():
    sharp = np.where(np.eye(4, dtype=bool), 1.0 - 3e-30, 1e-30)
    got = snp_variants_reference([[0.0, 0.0, 40.0, 0.0], [3.0, 2.0, 2.5, 2.0]], [1, 1], [2, 2], sharp, 0.5)
    assert got["best"].tolist() == [2, 0] and got["qual"][0] == 93 and 0 < got["qual"][1] < 93   # (-10 log10 3e-30 = 295)
    assert len(got["call_row"]) == 0 or got["call_row"].tolist() == [1]


def test_exact_ties_go_to_the_reference_base_else_to_the_lowest_code():
    """All weight on observed T; candidates C and G have the same entry for T and a flat evolution: their lp are the same number."""
    error = np.array([[0.7, 0.1, 0.1, 0.1], [0.1, 0.3, 0.2, 0.4], [0.1, 0.2, 0.3, 0.4], [0.25, 0.25, 0.25, 0.25]])
    weights = [[0.0, 0.0, 0.0, 7.0]] * 3
    got = snp_variants_reference(weights, [1, 1, 1], [2, 1, 0], error, 0.3)
    assert got["lp_gap"] == 0.0
    assert got["best"].tolist() == [2, 1, 1]     # reference G is among the tied; reference C is; reference A is not: the lowest code, C
    p = 0.4 / (0.1 + 0.4 + 0.4 + 0.25)
    assert got["qual"].tolist() == [int(np.floor(-10 * np.log10(1 - p)))] * 3
    assert list(zip(got["call_row"].tolist(), got["call_alt"].tolist())) == [(0, 1), (1, 2), (2, 1), (2, 2)]
    assert np.allclose(got["call_p"], p, rtol=1e-14, atol=0)


def test_guard_distances():
    got = snp_variants_reference([[2.0, 1.0, 1.0, 0.0]], [1], [0], FLAT, 0.25)
    lp = np.array([np.log(FLAT[c]) @ np.array([0.5, 0.25, 0.25, 0.0]) for c in range(4)])
    p = np.exp(lp) / np.exp(lp).sum()
    assert np.isclose(got["threshold_gap"], np.abs(p[1:] - 0.25).min(), rtol=1e-12)
    assert np.isclose(got["lp_gap"], np.sort(lp)[3] - np.sort(lp)[2], rtol=1e-12)
    phred = -10 * np.log10(1 - p[0])
    assert np.isclose(got["qual_gap"], abs(phred - round(phred)), rtol=1e-9)
    empty = snp_variants_reference(np.zeros((0, 4)), [], [], FLAT, 0.5)
    assert empty["threshold_gap"] == empty["lp_gap"] == empty["qual_gap"] == np.inf and len(empty["best"]) == 0


def test_writers_byte_for_byte():
    from nanopore_amd.analyses.consensus import callQuality, consensusFastq, consensusVcf
    names, lengths = ["chrA", "chrB"], [5, 3]
    best = np.array([0, 1, 4, 3, 2, 2, 4, 0], dtype=np.uint8)
    qual = np.array([0, 12, 0, 93, 40, 1, 0, 60], dtype=np.uint8)
    assert consensusFastq(names, lengths, best, qual) == "@chrA\nACNTG\n+\n!-!~I\n@chrB\nGNA\n+\n\"!]\n"
    ref_codes = np.array([0, 0, 4, 3, 1, 2, 2, 3], dtype=np.uint8)
    text = consensusVcf(names, lengths, ref_codes, [1, 1, 4, 5, 7], [1, 3, 2, 0, 0], [0.9, 0.5, 1.0, 0.998, 0.75])
    assert text == ("##fileformat=VCFv4.1\n"
                    "##contig=<ID=chrA,length=5>\n"
                    "##contig=<ID=chrB,length=3>\n"
                    "##INFO=<ID=PP,Number=1,Type=Float,Description=\"Posterior probability of the alternative base\">\n"
                    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
                    "chrA\t2\t.\tA\tC\t10\t.\tPP=0.900000\n"
                    "chrA\t2\t.\tA\tT\t3\t.\tPP=0.500000\n"
                    "chrA\t5\t.\tC\tG\t93\t.\tPP=1.000000\n"
                    "chrB\t1\t.\tG\tA\t26\t.\tPP=0.998000\n"
                    "chrB\t3\t.\tT\tA\t6\t.\tPP=0.750000\n")
    assert consensusVcf(names, lengths, ref_codes, [], [], []).count("\n") == 5
    assert callQuality(1.0) == 93 and callQuality(1.0 - 1e-12) == 93 and callQuality(0.0) == 0 and callQuality(0.5) == 3


def test_binding_and_driver_know_the_feature():
    from nanopore_amd import _lib, pipeline, realign
    from nanopore_amd.analyses.abstractAnalysis import AbstractAnalysis
    from nanopore_amd.analyses.consensus import Consensus
    for name in ("npr_snp_variants_table", "npr_batch_snp_variants", "npr_pileup_snp_variants"):
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib.i64 and argtypes[-2] is _lib.i64
    assert all(hasattr(cls, name) for cls, name in ((realign.Context, "snp_variants_table"), (realign.Batch, "snp_variants"), (realign.Pileup, "snp_variants")))
    assert pipeline.resolveClasses("Consensus", "nanopore_amd.analyses", AbstractAnalysis) == [Consensus]
    assert Consensus not in pipeline.analyses and Consensus.threshold == 0.5
