"""The unmapped-read meta-analyses, the parts that need no GPU (nanopore/metaAnalyses/abstractUnmappedAnalysis.py,
unmappedLengthDistributionAnalysis.py, comparePerReadMappabilityByMapper.py, unmappedKmerAnalysis.py).

The yardstick of tests/test_gpu_unmapped.py lives here too: `experiment_tree` builds a small tree of experiments with
seeded mapping.sam files, and the `reference_*` functions restate the reference's loops literally -- Read objects, the
(qname, readFastqFile) dict, the three `run` bodies -- fed the reads in the order this project defines (files sorted by
path, records in file order).  The native join of FASTQ names and SAM QNAMEs (npr_names_mark) is checked against a dict."""
import itertools
import os
import re
from collections import Counter, OrderedDict
from math import log

import numpy as np
import pytest

from nanopore_amd import _lib, bioio, ingest, realign
from nanopore_amd.metaAnalyses.abstractUnmappedAnalysis import AbstractUnmappedMetaAnalysis
from nanopore_amd.metaAnalyses.comparePerReadMappabilityByMapper import ComparePerReadMappabilityByMapper
from nanopore_amd.metaAnalyses.unmappedKmerAnalysis import writeUnmappedCounts
from nanopore_amd.metaAnalyses.unmappedLengthDistributionAnalysis import UnmappedLengthDistributionAnalysis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1_READS = os.path.join(ROOT, "tests", "golden", "c1", "reads.fq")


# ---- the reference's definitions, restated ----

def mapped_qnames(samPath):
    """samIterator (drops RNAME "*") followed by `not record.is_unmapped`: the QNAMEs abstractUnmappedAnalysis.py:39-43 keeps."""
    with open(samPath, newline="") as f:
        for line in f:
            line = line.rstrip("\r\n")
            if not line or line.startswith("@"):
                continue
            cols = line.split("\t")
            if cols[2] != "*" and not int(cols[1]) & 4:
                yield cols[0]


class RefRead(object):
    """abstractUnmappedAnalysis.py:8-27."""

    def __init__(self, name, seq, readType, readFastqFile, mapRefPairs):
        self.seq, self.name, self.readType, self.readFastqFile, self.mapRefPairs = seq, name, readType, readFastqFile, mapRefPairs
        if mapRefPairs is not None:
            self.is_mapped = True
            self.mappers, self.references = set(mapRefPairs[0]), set(mapRefPairs[1])
        else:
            self.is_mapped = False
            self.mappers, self.references = None, None

    def get_map_ref_pair(self):
        if self.mapRefPairs is not None:
            for mapper, reference in zip(self.mapRefPairs[0], self.mapRefPairs[1]):
                yield (mapper, reference)


def reads_in_defined_order(experiments):
    """(name, readFastqFile, readType, seq) of every record: the distinct (file, type) pairs sorted, records in file order."""
    out = []
    for readFastqFile, readType in sorted({(e[0], e[1]) for e in experiments}):
        for name, seq, _ in bioio.fastqRead(readFastqFile):
            out.append((name.split()[0], readFastqFile, readType, seq))
    return out


def reference_reads(experiments):
    """abstractUnmappedAnalysis.py:37-51 over reads_in_defined_order instead of the set of :34."""
    mappedReads = dict()
    for readFastqFile, readType, referenceFastaFile, mapper, analyses, resultsDir in experiments:
        for qname in mapped_qnames(os.path.join(resultsDir, "mapping.sam")):
            if (qname, readFastqFile) not in mappedReads:
                mappedReads[(qname, readFastqFile)] = set()
            mappedReads[(qname, readFastqFile)].add((mapper.__name__, referenceFastaFile))
    reads = list()
    for name, readFastqFile, readType, seq in reads_in_defined_order(experiments):
        if (name, readFastqFile) in mappedReads:
            mappers, referenceFastaFiles = map(tuple, zip(*mappedReads[(name, readFastqFile)]))
            reads.append(RefRead(name, seq, readType, readFastqFile, (mappers, referenceFastaFiles)))
        else:
            reads.append(RefRead(name, seq, readType, readFastqFile, None))
    return reads


def reference_length_files(experiments, reads):
    """{file name: text} of unmappedLengthDistributionAnalysis.py:9-29."""
    out = {}
    for readType in {e[1] for e in experiments}:
        unmapped, mapped = [], []
        for read in reads:
            if read.is_mapped is True and read.readType == readType:
                mapped.append("{}\n".format(len(read.seq)))
            elif read.readType == readType:
                unmapped.append("{}\n".format(len(read.seq)))
        out[readType + "_unmapped.txt"], out[readType + "_mapped.txt"] = "".join(unmapped), "".join(mapped)
    for reference in {e[2] for e in experiments}:
        unmapped, mapped = [], []
        for read in reads:
            if read.is_mapped is True:
                mapped.append("{}\n".format(len(read.seq)))
            else:
                unmapped.append("{}\n".format(len(read.seq)))
        out[os.path.basename(reference) + "_unmapped.txt"], out[os.path.basename(reference) + "_mapped.txt"] = "".join(unmapped), "".join(mapped)
    return out


def reference_mappability_files(experiments, reads):
    """{file name: text} of comparePerReadMappabilityByMapper.py:11-25."""
    baseMappers = {re.findall("[A-Z][a-z]*", e[3].__name__)[0] for e in experiments}
    out = {}
    for readType in {e[1] for e in experiments}:
        sortedBaseMappers = [x for x in sorted(baseMappers) if x != "Combined"]
        text = ["Read\tReadFastqFile\t", "\t".join(sortedBaseMappers), "\n"]
        for read in reads:
            if read.readType == readType:
                tmp = OrderedDict([[x, 0] for x in sortedBaseMappers])
                if read.is_mapped is True:
                    for mapper, reference in read.get_map_ref_pair():
                        baseMapper = re.findall("[A-Z][a-z]*", mapper)[0]
                        if baseMapper != "Combined" and tmp[baseMapper] == 0:
                            tmp[baseMapper] = 1
                text += ["\t".join([read.name, os.path.basename(read.readFastqFile)] + list(map(str, tmp.values()))), "\n"]
        out[readType + "_perReadMappability.tsv"] = "".join(text)
    return out


def reference_kmer_files(experiments, reads, kmerSize):
    """{file name: text} of unmappedKmerAnalysis.py:12-48 (rows over products of kmerSize letters, where the reference hard-codes 5)."""
    def countKmers(seq):
        kmers = Counter()
        for i in range(kmerSize, len(seq)):
            if "N" not in seq[i - kmerSize:i]:
                kmers[seq[i - kmerSize:i]] += 1
        return kmers

    out = {}
    for readType in {e[1] for e in experiments}:
        mappedKmers, unmappedKmers = Counter(), Counter()
        for read in reads:
            if read.readType == readType and read.is_mapped:
                mappedKmers += countKmers(read.seq)
            elif read.readType == readType:
                unmappedKmers += countKmers(read.seq)
        out[readType + "_kmer_counts.txt"] = reference_kmer_table(mappedKmers, unmappedKmers, kmerSize)
    return out


def reference_kmer_table(mappedKmers, unmappedKmers, kmerSize):
    """unmappedKmerAnalysis.py:29-48 from two Counters over strings."""
    mappedSize, unmappedSize = sum(mappedKmers.values()), sum(unmappedKmers.values())
    text = ["kmer\tmappableCount\tmappableFraction\tunmappableCount\tunmappableFraction\tlogFoldChange\n"]
    for kmer in itertools.product("ATGC", repeat=kmerSize):
        kmer = "".join(kmer)
        if mappedSize > 0:
            mappedFraction = 1.0 * mappedKmers[kmer] / mappedSize
        else:
            mappedFraction = 0
        if unmappedSize > 0:
            unmappedFraction = 1.0 * unmappedKmers[kmer] / unmappedSize
        else:
            unmappedFraction = 0
        if unmappedFraction == 0:
            foldChange = "-Inf"
        elif mappedFraction == 0:
            foldChange = "Inf"
        else:
            foldChange = -log(mappedFraction / unmappedFraction)
        text.append("\t".join(map(str, [kmer, mappedKmers[kmer], mappedFraction, unmappedKmers[kmer], unmappedFraction, foldChange])) + "\n")
    return "".join(text)


# ---- a small tree of experiments ----

class LastParams(object):
    pass


class LastParamsRealign(object):
    pass


class BlasrParams(object):
    pass


class CombinedMapper(object):
    pass


MAPPERS = [LastParams, LastParamsRealign, BlasrParams, CombinedMapper]


def _random_seq(rng, n, alphabet="ACGT"):
    return "".join(np.array(list(alphabet))[rng.integers(0, len(alphabet), size=n)])


def experiment_tree(root, seed=5, with_c1=True, read_len=(0, 400)):
    """Two read types, two FASTQ files of one of them, two references, four mappers: 24 experiments, each with a mapping.sam
    in which every read of its FASTQ file has no line, an unmapped line, a mapped line (forward or reverse, sometimes with
    a secondary one) or a line with a reference but FLAG 4; plus lines of reads no FASTQ file has.  Upper-case ACGTN reads,
    except tests/golden/c1/reads.fq (with_c1), which has lower case."""
    rng = np.random.default_rng(seed)
    root = str(root)
    fastqs = []
    for fname, readType, n in (("a_2D.fq", "2D", 40), ("b_2D.fq", "2D", 25), ("template.fq", "template", 30)):
        path = os.path.join(root, fname)
        names = ["%s_read_%d" % (fname[0], i) for i in range(n)]
        names[3] = names[2] + "x"        # a name that another is a prefix of
        names[7] = names[6]              # a name twice, with different sequences
        lengths = [int(rng.integers(read_len[0], read_len[1])) for _ in range(n)]
        lengths[0], lengths[1], lengths[2] = 0, 5, 6
        with open(path, "w") as f:
            for name, ln in zip(names, lengths):
                seq = _random_seq(rng, ln, "ACGTACGTACGTN")
                f.write("@%s\n%s\n+\n%s\n" % (name, seq, "#" * ln))
        fastqs.append((path, readType))
    if with_c1:
        fastqs[1] = (C1_READS, "2D")
    references = []
    for fname in ("refA.fa", "refB.fa"):
        path = os.path.join(root, fname)
        with open(path, "w") as f:
            for c in range(2):
                f.write(">%s_contig%d\n%s\n" % (fname[:4], c, _random_seq(rng, 200)))
        references.append(path)
    experiments = []
    for (fq, readType), ref, mapper in itertools.product(fastqs, references, MAPPERS):
        resultsDir = os.path.join(root, "results", "%s_%s_%s" % (os.path.basename(fq), os.path.basename(ref), mapper.__name__))
        os.makedirs(resultsDir)
        contigs = [n.split()[0] for n, _ in bioio.fastaRead(ref)]
        lines = ["@SQ\tSN:%s\tLN:200" % c for c in contigs]
        names = [n.split()[0] for n, _, _ in bioio.fastqRead(fq)]
        for name in names + ["stranger_%d" % i for i in range(3)]:
            what = int(rng.integers(0, 24 if mapper is BlasrParams else 12))  # 3 .. 5: placed (Blasr places fewer reads); above: no line
            contig = contigs[int(rng.integers(0, 2))]
            if what == 1:
                lines.append("\t".join([name, "4", "*", "0", "0", "*", "*", "0", "0", "*", "*"]))
            elif what == 2:
                lines.append("\t".join([name, "20", contig, "5", "0", "10M", "*", "0", "0", "*", "*"]))
            elif 3 <= what <= 5:
                lines.append("\t".join([name, "16" if what == 4 else "0", contig, "11", "60", "4S10M2D3M", "*", "0", "0", "*", "*"]))
                if what == 5:
                    lines.append("\t".join([name, "256", contig, "31", "3", "8M", "*", "0", "0", "*", "*"]))
        with open(os.path.join(resultsDir, "mapping.sam"), "w", newline="") as f:
            f.write("".join(ln + ("\r\n" if mapper is LastParamsRealign else "\n") for ln in lines))
        experiments.append((fq, readType, ref, mapper, [], resultsDir))
    return experiments


# ---- npr_names_mark against a dict ----

def _names(rng, n_names):
    """Seeded names (some twice, some a prefix of another) inside a FASTQ-like text, with bytes between them."""
    names = ["r%d" % int(x) for x in rng.integers(0, 10 ** 6, size=n_names)]
    for i in range(0, n_names - 3, 7):
        names[i + 1] = names[i] + "1"    # a prefix of its neighbour
        names[i + 3] = names[i]          # twice
    text, spans = [], []
    at = 0
    for name in names:
        rec = "@%s some description\nACGT\n+\n####\n" % name
        spans.append((at + 1, at + 1 + len(name)))
        text.append(rec)
        at += len(rec)
    return names, np.frombuffer("".join(text).encode() or b"\0", dtype=np.uint8), np.array(spans, dtype=np.int64).reshape(-1, 2)


def _sam(path, rng, names, n_lines, line_end="\n"):
    """A seeded SAM file over the names, names no read has and names in another letter case: (QNAMEs a dict would keep, strangers)."""
    pool = names + [n + "_no" for n in names[:50]] + [n.upper() for n in names[:20]]
    lines = ["@HD\tVN:1.0", "@SQ\tSN:chr1\tLN:1000"]
    want, strangers = set(), 0
    known = set(names)
    for _ in range(n_lines):
        q = pool[int(rng.integers(0, len(pool)))] if pool else "nobody"
        flag = (0, 4, 16, 20, 256)[int(rng.integers(0, 5))]
        rname = "*" if rng.random() < 0.2 else "chr1"
        lines.append("\t".join([q, str(flag), rname, "7", "30", "*" if rname == "*" else "12M1I3M", "*", "0", "0", "*", "*"]))
        if rname != "*" and not flag & 4:
            want.add(q)
            strangers += q not in known
    with open(path, "w", newline="") as f:
        f.write("".join(ln + line_end for ln in lines))
    assert want == set(mapped_qnames(path))
    return want, strangers


def _names_case(tmp_path, rng, n_names, n_lines, line_end="\n"):
    names, names_text, spans = _names(rng, n_names)
    path = str(tmp_path / "case.sam")
    want, strangers = _sam(path, rng, names, n_lines, line_end)
    return names, names_text, spans, path, want, strangers


def _mark(names_text, spans, path, mark=None):
    sam = ingest.SamText(path)
    mark = np.zeros(len(spans), dtype=np.uint8) if mark is None else mark
    return mark, realign.names_mark(names_text, spans, sam.text, sam.span, sam.parse(), mark)


@pytest.mark.parametrize("n_names,n_lines,line_end", [(300, 400, "\n"), (300, 400, "\r\n"), (50, 0, "\n"), (0, 40, "\n"), (0, 0, "\n"), (1, 1, "\n")])
def test_names_mark_equals_a_dict(tmp_path, n_names, n_lines, line_end):
    rng = np.random.default_rng(1000 * n_names + n_lines)
    names, names_text, spans, path, want, strangers = _names_case(tmp_path, rng, n_names, n_lines, line_end)
    mark, got_strangers = _mark(names_text, spans, path)
    assert mark.tolist() == [int(n in want) for n in names]
    assert got_strangers == strangers
    if n_lines >= 400:
        assert 0 < mark.sum() < len(mark) and strangers > 0
        twice = [i for i in range(0, n_names - 3, 7) if mark[i]]
        assert twice and all(mark[i + 3] for i in twice)        # records of one name share the mark
        assert any(mark[i] != mark[i + 1] for i in range(0, n_names - 3, 7))  # a name and its prefix do not


def test_names_mark_ors_and_never_clears(tmp_path):
    rng = np.random.default_rng(77)
    names, names_text, spans = _names(rng, 200)
    path, path2 = str(tmp_path / "one.sam"), str(tmp_path / "two.sam")
    want, _ = _sam(path, rng, names, 150)
    want2, _ = _sam(path2, rng, names, 150)
    first, _ = _mark(names_text, spans, path)
    both, _ = _mark(names_text, spans, path2, first.copy())
    assert first.tolist() == [int(n in want) for n in names] and both.tolist() == [int(n in want or n in want2) for n in names]
    assert (both >= first).all() and both.sum() > first.sum()
    again, _ = _mark(names_text, spans, path, both.copy())
    assert again.tolist() == both.tolist()


def test_names_mark_refuses_a_broken_line(tmp_path):
    names_text = np.frombuffer(b"@a\nAC\n+\n##\n", dtype=np.uint8)
    spans = np.array([[1, 2]], dtype=np.int64)
    for bad in ("a\t0\tchr9\t7\t30\t5M\t*\t0\t0\t*\t*", "a\tzero\tchr1\t7\t30\t5M\t*\t0\t0\t*\t*"):
        path = str(tmp_path / "bad.sam")
        with open(path, "w") as f:
            f.write("@SQ\tSN:chr1\tLN:1000\na\t0\tchr1\t7\t30\t5M\t*\t0\t0\t*\t*\n" + bad + "\n")
        mark = np.zeros(1, dtype=np.uint8)
        with pytest.raises(realign.NprError) as e:
            _mark(names_text, spans, path, mark)
        assert e.value.code == _lib.ERR_INVALID and mark.tolist() == [0]


def test_names_mark_is_the_same_on_one_thread_and_on_eight(tmp_path, monkeypatch):
    rng = np.random.default_rng(4)
    names, names_text, spans, path, want, strangers = _names_case(tmp_path, rng, 5000, 6000)
    got = {}
    for threads in ("1", "8"):
        monkeypatch.setenv("NPR_HOST_THREADS", threads)
        got[threads] = _mark(names_text, spans, path)
    assert got["1"][0].tolist() == got["8"][0].tolist() == [int(n in want) for n in names]
    assert got["1"][1] == got["8"][1] == strangers


# ---- the analyses on a tree of experiments ----

def test_length_files_and_mappability_table_equal_the_restated_loops(tmp_path):
    experiments = experiment_tree(tmp_path)
    reads = reference_reads(experiments)
    assert {r.readType for r in reads} == {"2D", "template"} and any(r.is_mapped for r in reads) and not all(r.is_mapped for r in reads)
    out = tmp_path / "lengths"
    out.mkdir()
    UnmappedLengthDistributionAnalysis(str(out), experiments).run()
    want = reference_length_files(experiments, reads)
    assert sorted(os.listdir(str(out))) == sorted(want) and len(want) == 8
    for name, text in want.items():
        assert (out / name).read_text() == text, name
    assert want["2D_mapped.txt"] and want["2D_unmapped.txt"] and want["refA.fa_mapped.txt"] == want["refB.fa_mapped.txt"]
    out = tmp_path / "mappability"
    out.mkdir()
    ComparePerReadMappabilityByMapper(str(out), experiments).run()
    want = reference_mappability_files(experiments, reads)
    assert sorted(os.listdir(str(out))) == sorted(want) and len(want) == 2
    for name, text in want.items():
        assert (out / name).read_text() == text, name
    header, rows = want["2D_perReadMappability.tsv"].split("\n")[0], want["2D_perReadMappability.tsv"].split("\n")[1:-1]
    assert header == "Read\tReadFastqFile\tBlasr\tLast" and {tuple(r.split("\t")[2:]) for r in rows} == {("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")}
    assert {r.split("\t")[1] for r in rows} == {"a_2D.fq", "reads.fq"}


def test_the_lazy_reads_view_agrees_with_the_arrays(tmp_path):
    experiments = experiment_tree(tmp_path, with_c1=False)
    meta = AbstractUnmappedMetaAnalysis(str(tmp_path), experiments)
    assert [(rf.readFastqFile, rf.readType) for rf in meta.readFiles] == sorted({(e[0], e[1]) for e in experiments})
    assert meta.strangers == sum(q.startswith("stranger_") for e in experiments for q in mapped_qnames(os.path.join(e[5], "mapping.sam"))) > 0
    reads, want = list(meta.reads), reference_reads(experiments)
    assert len(reads) == len(want) == sum(len(rf.table) for rf in meta.readFiles) == 95
    flat = [(rf, i) for rf in meta.readFiles for i in range(len(rf.table))]
    for read, ref, (rf, i) in zip(reads, want, flat):
        assert (read.name, read.seq, read.readType, read.readFastqFile, read.is_mapped) == (ref.name, ref.seq, ref.readType, ref.readFastqFile, ref.is_mapped)
        assert read.mappers == ref.mappers and read.references == ref.references
        assert set(read.get_map_ref_pair()) == set(ref.get_map_ref_pair())
        assert read.is_mapped == bool(rf.is_mapped[i]) and len(read.seq) == rf.table.lengths[i] and read.name == rf.table.name(i)
        bases = {re.findall("[A-Z][a-z]*", m)[0] for m in (read.mappers or ())}
        assert bases == {b for b, mark in rf.mapped_by.items() if mark[i]}
    assert any(r.mappers and len(r.mappers) > 1 for r in reads) and any(r.references and len(r.references) > 1 for r in reads)


def test_fastq_table_gives_the_records_where_they_lie():
    t = ingest.FastqTable(C1_READS)
    want = [(n.split()[0], s) for n, s, _ in bioio.fastqRead(C1_READS)]
    assert len(t) == len(want) == 2 and t.lengths.tolist() == [len(s) for _, s in want]
    assert [(t.name(i), t.sequence(i)) for i in range(len(t))] == want
    assert t.name_span.flags.c_contiguous and t.seq_span.flags.c_contiguous and t.text.dtype == np.uint8


def test_the_kmer_table_writer_on_hand_made_tables(tmp_path):
    path = str(tmp_path / "t.txt")
    head = "kmer\tmappableCount\tmappableFraction\tunmappableCount\tunmappableFraction\tlogFoldChange\n"
    # bins A C G T and the bin of the windows with an N, which no size counts
    writeUnmappedCounts(path, [3, 0, 0, 1, 9], [1, 0, 5, 0, 7], 1)
    want = head + "A\t3\t0.75\t1\t%s\t%s\nT\t1\t0.25\t0\t0.0\t-Inf\nG\t0\t0.0\t5\t%s\tInf\nC\t0\t0.0\t0\t0.0\t-Inf\n" % (
        str(1.0 / 6), str(-log(0.75 / (1.0 / 6))), str(5.0 / 6))
    assert open(path).read() == want == reference_kmer_table(Counter(A=3, T=1), Counter(A=1, G=5), 1)
    writeUnmappedCounts(path, [0, 0, 0, 0, 4], [1, 0, 1, 0, 0], 1)   # nothing mapped: the fraction is the integer 0
    assert open(path).read() == head + "A\t0\t0\t1\t0.5\tInf\nT\t0\t0\t0\t0.0\t-Inf\nG\t0\t0\t1\t0.5\tInf\nC\t0\t0\t0\t0.0\t-Inf\n" == reference_kmer_table(
        Counter(), Counter(A=1, G=1), 1)
    writeUnmappedCounts(path, [2, 0, 0, 0, 0], [0, 0, 0, 0, 3], 1)   # nothing unmapped
    assert open(path).read() == head + "A\t2\t1.0\t0\t0\t-Inf\nT\t0\t0.0\t0\t0\t-Inf\nG\t0\t0.0\t0\t0\t-Inf\nC\t0\t0.0\t0\t0\t-Inf\n" == reference_kmer_table(
        Counter(A=2), Counter(), 1)
    rng = np.random.default_rng(2)
    mapped, unmapped = rng.integers(0, 4, size=4 ** 3 + 1), rng.integers(0, 4, size=4 ** 3 + 1)
    writeUnmappedCounts(path, mapped, unmapped, 3)
    kmers = ["".join(p) for p in itertools.product("ACGT", repeat=3)]
    assert open(path).read() == reference_kmer_table(Counter(dict(zip(kmers, mapped.tolist()))), Counter(dict(zip(kmers, unmapped.tolist()))), 3)
    assert open(path).read().split("\n")[1:4] != [] and [ln.split("\t")[0] for ln in open(path).read().split("\n")[1:5]] == ["AAA", "AAT", "AAG", "AAC"]
