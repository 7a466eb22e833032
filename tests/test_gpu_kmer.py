"""The k-mer tables on the device (include/nprealign.h: npr_kmer_counts, npr_align_indel_kmers, npr_batch_indel_kmers;
csrc/npr_kmer.hip) and the two analyses built on them: exact-integer parity with Counters over Python slices and with the
literal restatement of the reference's column walk (tests/test_kmer_host.py), exact text of the written tables."""
import os
from collections import Counter

import numpy as np
import pytest

from nanopore_amd import _lib, bioio
from nanopore_amd.realign import NprError
from test_kmer_host import (ROOT, columns, expected_all_bases, expected_indel_bases, fold, indel_kmer_counters, literal_walk, sam_records, table_of,
                            window_counter)

pytestmark = pytest.mark.gpu

C1 = os.path.join(ROOT, "tests", "golden", "c1")


def _random_seq(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes().decode()


def _big_window_table(seq, k):
    """window_counter for one sequence of several Mb, vectorised: the same bins from numpy."""
    code = np.full(256, 4, dtype=np.int64)
    for i, ch in enumerate("ACGT"):
        code[ord(ch)] = code[ord(ch.lower())] = i
    c = code[np.frombuffer(seq.encode(), dtype=np.uint8)]
    n = len(c) - k                                    # windows s[i - k : i], i in k .. len - 1
    t = np.zeros(4 ** k + 1, dtype=np.int64)
    if n <= 0:
        return t
    num, bad = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for j in range(k):
        num = 4 * num + (c[j:j + n] & 3)
        bad |= c[j:j + n] == 4
    np.add.at(t, np.where(bad, 4 ** k, num), 1)
    return t


def test_kmer_counts_equal_a_counter_over_slices(gpu_ctx):
    rng = np.random.default_rng(11)
    big = _random_seq(rng, 3 * 1000 * 1000 + 17, b"ACGTACGTACGTNacgt")
    assert _big_window_table(big[:5000], 5).tolist() == table_of(window_counter([big[:5000]], 5), 5).tolist()
    for k in (1, 5, 6):
        small = ["", "A", "ACGTAC"[:k - 1] if k > 1 else "", "ACGTAC"[:k], "ACGTACG"[:k + 1], "ACGTNNNNNNNNNNACGTACGTTGCA", "NNNNNNNN", "acgtacgtRYacgtTTGCA",
                 _random_seq(rng, 70, b"ACGTN"), "T" * 100, _random_seq(rng, 33), _random_seq(rng, 8191), _random_seq(rng, 8193, b"ACGTNacgtn")]
        want = table_of(window_counter(small, k), k)
        got = gpu_ctx.kmer_counts(small, k)
        assert got.dtype == np.int64 and got.tolist() == want.tolist(), k
        # a sequence of several Mb between short ones: many workgroups, lanes whose halo crosses a sequence boundary
        got = gpu_ctx.kmer_counts(small[:6] + [big] + small[6:], k)
        assert got.tolist() == (want + _big_window_table(big, k)).tolist(), k
        assert got.sum() == sum(max(0, len(s) - k) for s in small + [big])
    assert gpu_ctx.kmer_counts([], 5).sum() == 0 and gpu_ctx.kmer_counts(["", ""], 5).sum() == 0
    for k in (0, 7):
        with pytest.raises(NprError) as e:
            gpu_ctx.kmer_counts(["ACGTACGTACGT"], k)
        assert e.value.code == _lib.ERR_INVALID


def _windows(refs, reads, cigars, starts=None):
    return [(fold(refs[i][(starts[i][0] if starts else 0):]), fold(reads[i][(starts[i][1] if starts else 0):]), cigars[i]) for i in range(len(reads))]


def _check(gpu_ctx, refs, reads, cigars, k, starts=None):
    rd, rf = gpu_ctx.align_indel_kmers(refs, reads, cigars, k=k, start=starts)
    want_rd, want_rf = indel_kmer_counters(_windows(refs, reads, cigars, starts), k)
    assert rd.dtype == np.int64 and rd.tolist() == table_of(want_rd, k).tolist() and rf.tolist() == table_of(want_rf, k).tolist()
    return int(rd.sum()), int(rf.sum())


HAND_CIGARS = [
    [(2, 4), (0, 30), (1, 3)], [(1, 4), (0, 30), (2, 3)],                       # gaps at either end
    [(0, 20), (2, 1), (0, 2), (2, 7), (0, 20), (1, 2), (0, 3), (1, 1), (0, 9)],     # two gaps closer than k
    [(0, 10), (1, 3), (2, 2), (0, 10), (2, 2), (1, 3), (0, 10)],                  # an I directly followed by a D and the other way round
    [(0, 10), (1, 0), (2, 0), (0, 4), (2, 1), (0, 0), (2, 1), (0, 1), (1, 0), (0, 9)],  # zero-length operations, a gap in two pieces
    [(0, 3), (2, 1)] + [(0, 1)] * 70 + [(1, 2), (0, 5)] + [(0, 2)] * 80 + [(2, 3), (0, 7)],  # gaps more than 64 operations apart
    [op for i in range(150) for op in ((0, 1 + i % 7), (1 + i % 2, 1 + i % 3))] + [(0, 12)],  # more than 64 operations, a gap every few bases
    [(0, 4), (2, 2), (0, 4), (2, 2), (0, 4), (1, 1), (0, 1), (2, 5), (0, 2)], [(0, 40)], [], [(1, 5)], [(2, 5)],
]


@pytest.mark.parametrize("k", [3, 5])
def test_indel_kmers_equal_the_literal_walk(gpu_ctx, k):
    rng = np.random.default_rng(3)
    refs, reads, starts = [], [], []
    for cigar in HAND_CIGARS:
        x0, y0 = int(rng.integers(0, 9)), int(rng.integers(0, 9))
        refs.append(_random_seq(rng, x0 + sum(ln for op, ln in cigar if op != 1) + int(rng.integers(0, 5)), b"ACGTACGTNacgt"))
        reads.append(_random_seq(rng, y0 + sum(ln for op, ln in cigar if op != 2) + int(rng.integers(0, 5)), b"ACGTACGTNacgt"))
        starts.append((x0, y0))
    for i in range(len(HAND_CIGARS)):                 # one at a time, so that a wrong record is named
        assert _check(gpu_ctx, refs[i:i + 1], reads[i:i + 1], HAND_CIGARS[i:i + 1], k, starts[i:i + 1]) is not None, i
    n_rd, n_rf = _check(gpu_ctx, refs, reads, HAND_CIGARS, k, starts)
    assert n_rd > 100 and n_rf > 100
    for kk in (1, 2, 4, 6):
        _check(gpu_ctx, refs, reads, HAND_CIGARS, kk, starts)
    # a cigar that runs past its read: that record adds nothing, the call says so
    rd = np.zeros(4 ** k + 1, dtype=np.int64)
    rf = np.zeros(4 ** k + 1, dtype=np.int64)
    ref, ref_off = np.frombuffer(b"ACGTACGTACGTACGTACGT" * 2, dtype=np.uint8), np.array([0, 20, 40], dtype=np.int64)
    read, read_off = np.frombuffer(b"ACGTAGTACGTACGTACGTA" + b"ACGTACG", dtype=np.uint8), np.array([0, 20, 27], dtype=np.int64)
    ops, ops_off = np.array([[0, 5], [2, 1], [0, 14], [0, 4], [2, 2], [0, 6]], dtype=np.int32), np.array([0, 3, 6], dtype=np.int64)
    rc = gpu_ctx._L.npr_align_indel_kmers(gpu_ctx._h, k, 2, 2, _lib.ptr(ref), _lib.ptr(ref_off), None, _lib.ptr(read), _lib.ptr(read_off), _lib.ptr(ops),
                                          _lib.ptr(ops_off), None, _lib.ptr(rd), _lib.ptr(rf))
    want_rd, _ = indel_kmer_counters([("ACGTACGTACGTACGTACGT", "ACGTAGTACGTACGTACGTA", [(0, 5), (2, 1), (0, 14)])], k)
    assert rc == _lib.ERR_INVALID and rd.tolist() == table_of(want_rd, k).tolist() and rf.sum() == 0
    for bad_k in (0, 7):
        with pytest.raises(NprError):
            gpu_ctx.align_indel_kmers(refs, reads, HAND_CIGARS, k=bad_k, start=starts)


@pytest.mark.parametrize("k", [3, 5])
def test_indel_kmers_of_synthetic_records(gpu_ctx, k):
    from helpers import load_model_arrays
    from nanopore_amd import synth
    T, E, _ = load_model_arrays()
    w = synth.make_workload(41, 3000, 600, T, E, flank=0, length_sigma=0.5, len_min=20, len_max=3000)
    rng = np.random.default_rng(9)
    ref, read = w["ref"].copy(), w["read"].copy()
    ref[rng.random(len(ref)) < 0.01] = ord("N")
    read[rng.random(len(read)) < 0.01] = ord("n")
    refs = [bytes(ref[w["ref_off"][i]:w["ref_off"][i + 1]]).decode() for i in range(3000)]
    reads = [bytes(read[w["read_off"][i]:w["read_off"][i + 1]]).decode() for i in range(3000)]
    go = w["guide_ops"].reshape(-1, 2)
    cigars = [[(int(a), int(c)) for a, c in go[w["guide_off"][i]:w["guide_off"][i + 1]]] for i in range(3000)]
    n_rd, n_rf = _check(gpu_ctx, refs, reads, cigars, k)
    assert n_rd > 10000 and n_rf > 10000


def test_indel_kmers_of_a_realigned_batch_where_it_lies(gpu_ctx):
    """npr_batch_indel_kmers == npr_align_indel_kmers on the cigars npr_batch_ops returns, reads with several segments."""
    from helpers import MODEL_DIR, load_model_arrays
    from nanopore_amd import realign as R, synth
    from nanopore_amd.hmm import Hmm
    T, E, _ = load_model_arrays()
    w = synth.make_workload(77, 64, 1500, T, E, flank=0, length_sigma=0.4, len_min=200, len_max=4000)
    gpu_ctx.set_hmm(Hmm.loadHmm(MODEL_DIR + "/blasr_hmm_0.txt"))
    read = w["read"].copy()
    read[::53] = ord("N")
    P = R.make_params(band_mode=R.BAND_ANCHOR, constraint_trim=4, split_threshold=100, max_pairs_per_base=40)
    for host_mea in (False, True):
        if host_mea:
            gpu_ctx.set_option(_lib.OPTIONS["host_mea"], 1)
        b = gpu_ctx.stage_csr(P, w["ref"], w["ref_off"], read, w["read_off"], w["guide_ops"], w["guide_off"])
        with pytest.raises(NprError) as e:
            b.indel_kmers(5)
        assert e.value.code == _lib.ERR_STATE
        b.run(), b.finish()
        res, (off, ops) = b.results(), b.ops()
        assert (res["status"] == 0).all() and res["n_segments"].max() > 1
        refs = [bytes(w["ref"][w["ref_off"][i]:w["ref_off"][i + 1]]).decode() for i in range(64)]
        reads = [bytes(read[w["read_off"][i]:w["read_off"][i + 1]]).decode() for i in range(64)]
        cigars = [[(int(a), int(c)) for a, c in ops[off[i]:off[i + 1]]] for i in range(64)]
        for k in (3, 5):
            got = b.indel_kmers(k)
            want = gpu_ctx.align_indel_kmers(refs, reads, cigars, k=k)
            assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[0].sum() > 1000 and got[1].sum() > 1000
        want_rd, want_rf = indel_kmer_counters(_windows(refs, reads, cigars), 5)
        assert got[0].tolist() == table_of(want_rd, 5).tolist() and got[1].tolist() == table_of(want_rf, 5).tolist()
        with pytest.raises(NprError):
            b.indel_kmers(7)
        b.close()
        gpu_ctx.set_option(_lib.OPTIONS["host_mea"], 0)


def test_analyses_on_the_reference_test_data(tmp_path, gpu_ctx):
    from nanopore_amd.analyses.indelKmerAnalysis import IndelKmerAnalysis
    from nanopore_amd.analyses.kmerAnalysis import KmerAnalysis
    fa, fq = os.path.join(C1, "reference.fa"), os.path.join(C1, "reads.fq")
    refs = [(n.split()[0], s) for n, s in bioio.fastaRead(fa)]
    reads = [(n.split()[0], s) for n, s, _ in bioio.fastqRead(fq)]
    # a small SAM over them: a clipped record with gaps of both kinds, a reverse-strand one, one without a reference
    (rname, rseq), (q1, s1), (q2, s2) = refs[0], reads[0], reads[1]
    m = min(len(s1) - 12, 180)
    lines = [[q1, "0", rname, "101", "60", "4S30M3D%dM2I20M1D6M%dS" % (m - 78, len(s1) - m - 4 + 20), "*", "0", "0", s1, "*"],
             [q2, "16", rname, "2001", "60", "25M4I30M2D10M%dS" % (len(s2) - 69), "*", "0", "0", s2, "*"],
             [q2, "4", "*", "0", "0", "*", "*", "0", "0", s2, "*"]]
    samp = tmp_path / "mapping.sam"
    samp.write_text("".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in refs) + "".join("\t".join(ln) + "\n" for ln in lines))
    records = sam_records(str(samp), fa)
    assert len(records) == 2
    for k in (5, 3):
        out = tmp_path / ("kmer%d" % k)
        out.mkdir()
        KmerAnalysis(fq, "2D", fa, str(samp), str(out)).run(kmerSize=k, ctx=gpu_ctx)
        assert (out / "all_bases_kmer_counts.txt").read_text() == expected_all_bases([s for _, s in refs], [s for _, s in reads], k)
        assert (out / "DONE").exists()
        out2 = tmp_path / ("indel%d" % k)
        out2.mkdir()
        IndelKmerAnalysis(fq, "2D", fa, str(samp), str(out2)).run(kmerSize=k, ctx=gpu_ctx)
        want = expected_indel_bases(records, k)
        assert want is not None and (out2 / "indel_bases_kmer_counts.txt").read_text() == want and (out2 / "DONE").exists()
