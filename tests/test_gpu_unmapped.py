"""The grouped k-mer count on the device (include/nprealign.h: npr_kmer_counts_groups; csrc/npr_kmer.hip:
k_kmer_spectrum_groups) and UnmappedKmerAnalysis built on it: exact-integer parity, bin for bin, with Counters over Python
slices per group and with the one-table kernel (ctx.kmer_counts) on each group's sequences alone; exact text of the tables
against the restated loops of the reference (tests/test_unmapped_host.py)."""
import numpy as np
import pytest

from nanopore_amd import _lib, ingest
from nanopore_amd.realign import NprError
from test_kmer_host import table_of, window_counter
from test_unmapped_host import experiment_tree, reference_kmer_files, reference_reads

pytestmark = pytest.mark.gpu

TILE = 8192  # bases a workgroup of the kernel takes per step: a group's bases start on a multiple of it


def _random_seq(rng, n, alphabet="ACGT"):
    return np.frombuffer(alphabet.encode(), dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes().decode()


def _sequences(rng, k, n_groups):
    """[(sequence, group)], shuffled: the short and odd ones spread over all groups and -1; group 0 and the last group with
    several tiles of bases, one ending exactly on a tile; group 1 of seven or more without any sequence; the others far below a tile."""
    odd = ["", "", "ACGTAC"[:k], "ACGTACG"[:k + 1], "GATTACA"[:k - 1] if k > 1 else "", "acgtacgtnnACGTRYKMSWacgtTTGCAacgt" * 3, "N" * 40, "ACGTNNNNNNNNNNACGTACGTTGCA",
           "T" * 300, _random_seq(rng, 70, "ACGTN"), _random_seq(rng, 500, "ACGTNacgtn"), _random_seq(rng, 33)]
    usable = [g for g in range(n_groups) if not (n_groups >= 7 and g == 1)]
    out = [(s, usable[i % len(usable)]) for i, s in enumerate(odd)] + [(s, usable[(i * 5 + 3) % len(usable)]) for i, s in enumerate(odd)]
    out += [(s, -1) for s in odd[2:8]] + [(_random_seq(rng, 3000), -1)]
    for g in {0, n_groups - 1}:
        lens = [int(x) for x in rng.integers(200, 3000, size=24)]
        out += [(_random_seq(rng, n, "ACGTACGTACGTACGTN"), g) for n in lens]
    if n_groups >= 2:  # the last group ends exactly on a tile boundary
        have = sum(len(s) for s, g in out if g == n_groups - 1)
        out.append((_random_seq(rng, (-have) % TILE + TILE), n_groups - 1))
    for g in usable[1:-1]:
        out += [(_random_seq(rng, int(rng.integers(1, 400)), "ACGTacgtN"), g) for _ in range(int(rng.integers(0, 3)))]
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def _as_fastq(tmp_path, tagged):
    """The sequences as a FASTQ file, read back where they lie: (text, begin, end) with header, '+' and quality lines between the spans."""
    path = str(tmp_path / "reads.fq")
    with open(path, "w") as f:
        for i, (s, _) in enumerate(tagged):
            f.write("@r%d ACGTACGTACGT\n%s\n+\n%s\n" % (i, s, "A" * len(s)))   # (quality letters that would count if a span slipped)
    t = ingest.FastqTable(path)
    assert [t.sequence(i) for i in range(len(t))] == [s for s, _ in tagged]
    return t.text, t.seq_span[:, 0], t.seq_span[:, 1]


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_groups_equal_counters_over_slices_and_the_one_table_kernel(tmp_path, gpu_ctx, k):
    for n_groups in (1, 2, 7, 64):
        rng = np.random.default_rng(100 * k + n_groups)
        tagged = _sequences(rng, k, n_groups)
        text, begin, end = _as_fastq(tmp_path, tagged)
        group = np.array([g for _, g in tagged], dtype=np.int32)
        got = gpu_ctx.kmer_counts_groups(text, begin, end, group, n_groups, k)
        assert got.dtype == np.int64 and got.shape == (n_groups, 4 ** k + 1)
        bases = [sum(len(s) for s, gg in tagged if gg == g) for g in range(n_groups)]
        assert bases[0] > 3 * TILE and bases[-1] > 3 * TILE and (n_groups < 2 or bases[-1] % TILE == 0)
        assert n_groups < 7 or (bases[1] == 0 and 0 < min(b for b in bases if b) < TILE)
        for g in range(n_groups):
            mine = [s for s, gg in tagged if gg == g]
            assert got[g].tolist() == table_of(window_counter(mine, k), k).tolist(), (n_groups, g)
            assert got[g].tolist() == gpu_ctx.kmer_counts(mine, k).tolist(), (n_groups, g)
            assert got[g].sum() == sum(max(0, len(s) - k) for s in mine)
        again = gpu_ctx.kmer_counts_groups(text, begin, end, group, n_groups, k)   # nothing of the first call is left in the context
        assert again.tolist() == got.tolist()
    none = gpu_ctx.kmer_counts_groups(np.zeros(0, dtype=np.uint8), [], [], [], 3, k)
    assert none.shape == (3, 4 ** k + 1) and none.sum() == 0
    short = gpu_ctx.kmer_counts_groups(np.frombuffer(b"ACGTACGTAC", dtype=np.uint8), [0, 3, 3], [k, 3, 3 + k], [0, 1, 1], 2, k)
    assert short.sum() == 0


def _vector_table(seq, k):
    """The table of one long sequence from numpy (the same bins as a Counter over its slices, without two million of them)."""
    code = np.full(256, 4, dtype=np.int64)
    for i, ch in enumerate("ACGT"):
        code[ord(ch)] = code[ord(ch.lower())] = i
    c = code[np.frombuffer(seq.encode(), dtype=np.uint8)]
    n = len(c) - k
    num, bad = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for j in range(k):
        num = 4 * num + (c[j:j + n] & 3)
        bad |= c[j:j + n] == 4
    t = np.zeros(4 ** k + 1, dtype=np.int64)
    np.add.at(t, np.where(bad, 4 ** k, num), 1)
    return t


def test_a_hot_bin_beside_a_random_group(gpu_ctx):
    rng = np.random.default_rng(21)
    n = 1 << 20
    poly, rand = "A" * n, _random_seq(rng, n, "ACGTACGTACGTN")
    assert _vector_table(rand[:4000], 5).tolist() == table_of(window_counter([rand[:4000]], 5), 5).tolist()
    text = np.frombuffer((poly + rand).encode(), dtype=np.uint8)
    for k in (1, 5, 6):
        got = gpu_ctx.kmer_counts_groups(text, [0, n], [n, 2 * n], [1, 0], 2, k)
        want_poly = np.zeros(4 ** k + 1, dtype=np.int64)
        want_poly[0] = n - k
        assert got[1].tolist() == want_poly.tolist()
        assert got[0].tolist() == _vector_table(rand, k).tolist() == gpu_ctx.kmer_counts([rand], k).tolist()


def test_bad_arguments_leave_the_tables_alone(gpu_ctx):
    text = np.frombuffer(b"ACGTACGTACGTACGTACGT", dtype=np.uint8)
    begin, end = np.array([0, 10], dtype=np.int64), np.array([10, 20], dtype=np.int64)

    def call(k, group, n_groups, b=begin, e=end):
        out = np.full(64 * (4 ** 6 + 1), -7, dtype=np.int64)
        group = np.array(group, dtype=np.int32)
        rc = gpu_ctx._L.npr_kmer_counts_groups(gpu_ctx._h, k, 2, _lib.ptr(text), _lib.ptr(b), _lib.ptr(e), _lib.ptr(group), n_groups, _lib.ptr(out))
        return rc, out

    for k, group, n_groups in ((5, [0, 2], 2), (5, [-2, 0], 2), (5, [0, 64], 64), (5, [0, 0], 0), (5, [0, 0], 65), (5, [0, 0], -1), (0, [0, 1], 2), (7, [0, 1], 2)):
        rc, out = call(k, group, n_groups)
        assert rc == _lib.ERR_INVALID and (out == -7).all(), (k, group, n_groups)
    rc, out = call(5, [0, 1], 2, np.array([0, 12], dtype=np.int64), np.array([10, 11], dtype=np.int64))   # a span that ends before it begins
    assert rc == _lib.ERR_INVALID and (out == -7).all()
    rc, out = call(5, [1, -1], 2)
    nb = 4 ** 5 + 1
    assert rc == _lib.OK and out[:nb].sum() == 0 and out[nb:2 * nb].sum() == 5 and (out[2 * nb:] == -7).all()
    for k, n_groups in ((0, 2), (7, 2), (5, 0), (5, 65)):
        with pytest.raises(NprError) as e:
            gpu_ctx.kmer_counts_groups(text, begin, end, [0, 0], n_groups, k)
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(NprError):
        gpu_ctx.kmer_counts_groups(text, begin, [10, 21], [0, 0], 2, 5)   # past the text: refused before the library sees it


def test_unmapped_kmer_analysis_end_to_end(tmp_path, gpu_ctx):
    from nanopore_amd.metaAnalyses.unmappedKmerAnalysis import UnmappedKmerAnalysis
    tree = tmp_path / "tree"
    tree.mkdir()
    experiments = experiment_tree(tree, seed=9, with_c1=False, read_len=(0, 2500))
    reads = reference_reads(experiments)
    assert all(set(r.seq) <= set("ACGTN") for r in reads) and sum(len(r.seq) for r in reads) > 10 * TILE
    for k in (5, 3):
        out = tmp_path / ("out%d" % k)
        out.mkdir()
        UnmappedKmerAnalysis(str(out), experiments).run(kmerSize=k, ctx=gpu_ctx)
        want = reference_kmer_files(experiments, reads, k)
        assert sorted(p.name for p in out.iterdir()) == sorted(want) == ["2D_kmer_counts.txt", "template_kmer_counts.txt"]
        for name, text in want.items():
            assert (out / name).read_text() == text, (k, name)
            rows = [ln.split("\t") for ln in text.split("\n")[1:-1]]
            assert len(rows) == 4 ** k and sum(int(r[1]) for r in rows) > 1000 and sum(int(r[3]) for r in rows) > 1000
