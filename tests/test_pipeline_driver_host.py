"""The pipeline driver (nanopore_amd/pipeline.py) and the plugins that came with it, on the host: no test here needs a device.

  * the driver on a stub mapper and stub analyses: the directory tree, resuming, re-mapping, a failing analysis
  * makeFastqSequenceNamesUnique / makeFastaSequenceNamesUnique
  * Hmm and HmmMetaAnalysis on hmm.txt.xml files written by em.writeXML from hand-made trial models
  * ChannelMappability, CoverageSummary on hand-written inputs
"""
import os
import re
import shutil
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from nanopore_amd import em, pipeline
from nanopore_amd.analyses.abstractAnalysis import AbstractAnalysis
from nanopore_amd.analyses.channelMappability import ChannelMappability
from nanopore_amd.analyses.hmmAnalysis import Hmm as HmmAnalysis
from nanopore_amd.analyses.names import makeFastaSequenceNamesUnique, makeFastqSequenceNamesUnique
from nanopore_amd.hmm import Hmm
from nanopore_amd.mappers.abstractMapper import AbstractMapper
from nanopore_amd.metaAnalyses.comparePerReadMappabilityByMapper import ComparePerReadMappabilityByMapper
from nanopore_amd.metaAnalyses.coverageSummary import COLUMNS, CoverageSummary
from nanopore_amd.metaAnalyses.hmmMetaAnalysis import HmmMetaAnalysis

BASES = "ACGT"


# ---- the driver ----

CALLS = {"mapper": [], "analysis": []}   # what the stubs ran: experiment directory names, (experiment, analysis class) pairs
FAIL_IN = []                             # StubSecond raises in experiment directories whose name ends with one of these
PREPARED = {}                            # reference basename -> a SAM prepared for it


class StubMapper(AbstractMapper):
    def run(self):
        CALLS["mapper"].append(os.path.basename(os.path.dirname(self.outputSamFile)))
        assert self.emptyHmmFile == os.path.join(os.path.dirname(self.outputSamFile), "hmm.txt")
        assert "processedReadFastqFiles" in self.readFastqFile and "processedReferenceFastaFiles" in self.referenceFastaFile
        shutil.copyfile(PREPARED[os.path.basename(self.referenceFastaFile)], self.outputSamFile)


class StubMapperChain(StubMapper):
    pass


class StubMapperRealign(StubMapper):
    pass


class StubFirst(AbstractAnalysis):
    def run(self):
        experiment = os.path.basename(os.path.dirname(self.outputDir))
        CALLS["analysis"].append((experiment, type(self).__name__))
        assert self.samFile == os.path.join(os.path.dirname(self.outputDir), "mapping.sam") and os.path.isfile(self.samFile)
        if type(self) is StubSecond and any(experiment.endswith(e) for e in FAIL_IN):
            raise ValueError("stub analysis told to fail")
        with open(os.path.join(self.outputDir, "marker.txt"), "w") as fh:
            fh.write(self.readType)
        self.finish()


class StubSecond(StubFirst):
    pass


def _working_dir(root):
    """Two read types with a read file each, two references, and files the driver has to leave alone."""
    for sub in ("readFastqFiles/typeA", "readFastqFiles/typeB", "referenceFastaFiles", "prepared"):
        os.makedirs(os.path.join(str(root), sub))
    seq = "ACGTTGCAAGGCTTAACCGT"
    for path, names in (("readFastqFiles/typeA/one.fq", ("r1 first", "r2", "r1")), ("readFastqFiles/typeB/two.fastq", ("s1", "s2"))):
        with open(os.path.join(str(root), path), "w") as fh:
            for n in names:
                fh.write("@%s\n%s\n+\n%s\n" % (n, seq, "I" * len(seq)))
    for path, name in (("ref1.fa", "contigA some words"), ("ref2.fasta", "contigB")):
        with open(os.path.join(str(root), "referenceFastaFiles", path), "w") as fh:
            fh.write(">%s\n%s\n%s\n" % (name, seq, seq))
        sam = os.path.join(str(root), "prepared", path + ".sam")
        with open(sam, "w") as fh:
            fh.write("@SQ\tSN:%s\tLN:%d\n" % (name.split()[0], 2 * len(seq)))
            fh.write("\t".join(["r2", "0", name.split()[0], "1", "255", "%dM" % len(seq), "*", "0", "0", seq, "*"]) + "\n")
        PREPARED[path] = sam
    for path in ("readFastqFiles/typeA/notes.txt", "readFastqFiles/stray.fq", "referenceFastaFiles/ref1.fa.fai"):
        with open(os.path.join(str(root), path), "w") as fh:
            fh.write("not an input\n")
    return str(root)


EXPERIMENTS = {"analysis_%s/experiment_%s_%s_%s" % (t, q, a, m)
               for t, q in (("typeA", "one.fq"), ("typeB", "two.fastq")) for a in ("ref1.fa", "ref2.fasta") for m in ("StubMapperChain", "StubMapperRealign")}
META = {"metaAnalysis_CoverageSummary", "metaAnalysis_HmmMetaAnalysis", "metaAnalysis_ComparePerReadMappabilityByMapper"}


@pytest.fixture
def stubs(monkeypatch):
    monkeypatch.setattr(pipeline, "mappers", [StubMapperChain, StubMapperRealign])
    monkeypatch.setattr(pipeline, "analyses", [StubFirst, StubSecond])
    monkeypatch.setattr(pipeline, "metaAnalyses", [CoverageSummary, HmmMetaAnalysis, ComparePerReadMappabilityByMapper])
    CALLS["mapper"], CALLS["analysis"], FAIL_IN[:] = [], [], []
    yield
    FAIL_IN[:] = []


def _directories(output):
    """Every directory below output/, relative, down to the analysis directories."""
    found = set()
    for base, dirs, _ in os.walk(output):
        found.update(os.path.relpath(os.path.join(base, d), output) for d in dirs)
    return found


def test_driver_lays_out_resumes_and_remaps(tmp_path, stubs):
    work = _working_dir(tmp_path)
    assert pipeline.main([work]) == 0
    output = os.path.join(work, "output")
    want = set(EXPERIMENTS) | {e + "/analysis_" + a for e in EXPERIMENTS for a in ("StubFirst", "StubSecond")} | META
    want |= {"analysis_typeA", "analysis_typeB", "processedReadFastqFiles", "processedReadFastqFiles/typeA", "processedReadFastqFiles/typeB",
             "processedReferenceFastaFiles"}
    assert _directories(output) == want
    assert sorted(os.listdir(os.path.join(output, "processedReadFastqFiles", "typeA"))) == ["one.fq"]
    assert sorted(os.listdir(os.path.join(output, "processedReferenceFastaFiles"))) == ["ref1.fa", "ref2.fasta"]
    assert open(os.path.join(output, "processedReadFastqFiles", "typeA", "one.fq")).read().split("\n")[0::4][:3] == ["@r1", "@r2", "@r1_1"]
    assert open(os.path.join(output, "processedReferenceFastaFiles", "ref1.fa")).readline() == ">contigA\n"
    # every experiment mapped once, in the order read type, read file, reference, mapper; both analyses after each mapping
    order = ["experiment_%s_%s_%s" % (q, a, m) for q in ("one.fq", "two.fastq") for a in ("ref1.fa", "ref2.fasta") for m in ("StubMapperChain", "StubMapperRealign")]
    assert CALLS["mapper"] == order
    assert CALLS["analysis"] == [(e, a) for e in order for a in ("StubFirst", "StubSecond")]
    for e in EXPERIMENTS:
        assert os.path.isfile(os.path.join(output, e, "mapping.sam"))
        for a in ("StubFirst", "StubSecond"):
            assert AbstractAnalysis.isFinished(os.path.join(output, e, "analysis_" + a))
            assert open(os.path.join(output, e, "analysis_" + a, "marker.txt")).read() == e.split("/")[0][len("analysis_"):]
    # the meta-analyses saw the experiments: which reads the stub "mapped"
    table = open(os.path.join(output, "metaAnalysis_ComparePerReadMappabilityByMapper", "typeA_perReadMappability.tsv")).read()
    assert table == "Read\tReadFastqFile\tStub\nr1\tone.fq\t0\nr2\tone.fq\t1\nr1_1\tone.fq\t0\n"

    # a second run: nothing is mapped, nothing analysed
    assert pipeline.main([work]) == 0
    assert len(CALLS["mapper"]) == 8 and len(CALLS["analysis"]) == 16
    assert _directories(output) == want

    # one mapping.sam gone: that experiment's mapper and both its analyses run again, nothing else
    gone = "experiment_two.fastq_ref1.fa_StubMapperRealign"
    os.remove(os.path.join(output, "analysis_typeB", gone, "mapping.sam"))
    assert pipeline.main([work]) == 0
    assert CALLS["mapper"][8:] == [gone]
    assert CALLS["analysis"][16:] == [(gone, "StubFirst"), (gone, "StubSecond")]
    assert os.path.isfile(os.path.join(output, "analysis_typeB", gone, "mapping.sam"))

    # an unfinished analysis of a mapped experiment: that analysis alone
    AbstractAnalysis.reset(os.path.join(output, "analysis_typeA", order[0], "analysis_StubSecond"))
    assert pipeline.main([work]) == 0
    assert len(CALLS["mapper"]) == 9 and CALLS["analysis"][18:] == [(order[0], "StubSecond")]


def test_driver_finishes_the_rest_when_an_experiment_fails(tmp_path, stubs):
    work = _working_dir(tmp_path)
    output = os.path.join(work, "output")
    bad = "experiment_one.fq_ref2.fasta_StubMapperChain"
    FAIL_IN.append(bad)
    with pytest.raises(RuntimeError, match="Got failed jobs") as raised:
        pipeline.main([work])
    assert os.path.join(output, "analysis_typeA", bad) in str(raised.value)
    assert len(re.findall("experiment_", str(raised.value).split("Analyses failed")[0])) == 1   # one failed directory is named, no other
    assert len(CALLS["mapper"]) == 8 and len(CALLS["analysis"]) == 16
    for e in EXPERIMENTS:
        for a in ("StubFirst", "StubSecond"):
            finished = not (e.endswith(bad) and a == "StubSecond")   # (the failing analysis' sibling ran as well)
            assert AbstractAnalysis.isFinished(os.path.join(output, e, "analysis_" + a)) == finished
            assert os.path.isfile(os.path.join(output, e, "analysis_" + a, "marker.txt")) == finished
    assert all(os.path.isdir(os.path.join(output, m)) for m in META)
    assert os.path.isfile(os.path.join(output, "metaAnalysis_ComparePerReadMappabilityByMapper", "typeB_perReadMappability.tsv"))
    # with the cause gone, the next run does what is left: that one analysis
    FAIL_IN[:] = []
    assert pipeline.main([work]) == 0
    assert len(CALLS["mapper"]) == 8 and CALLS["analysis"][16:] == [(bad, "StubSecond")]


def test_driver_removes_the_sam_of_a_mapper_that_raised(tmp_path, stubs, monkeypatch):
    class StubMapperBroken(StubMapper):
        def run(self):
            StubMapper.run(self)
            raise ValueError("stub mapper told to fail")

    monkeypatch.setattr(pipeline, "mappers", [StubMapperBroken])
    monkeypatch.setattr(pipeline, "metaAnalyses", [CoverageSummary])
    work = _working_dir(tmp_path)
    with pytest.raises(RuntimeError, match="Got failed jobs"):
        pipeline.main([work])
    assert len(CALLS["mapper"]) == 4 and CALLS["analysis"] == []          # no analysis of a mapping that failed
    for base, _, files in os.walk(os.path.join(work, "output")):
        assert "mapping.sam" not in files


def test_driver_resolves_class_names():
    from nanopore_amd.analyses.coverage import GlobalCoverage
    from nanopore_amd.mappers import variants
    from nanopore_amd.metaAnalyses.abstractMetaAnalysis import AbstractMetaAnalysis
    from nanopore_amd.metaAnalyses.coverageDepth import CoverageDepth
    assert [m.__name__ for m in pipeline.mappers] == ["SeedMapperChain", "SeedMapperRealign", "SeedMapperRealignEm"]
    assert [a.__name__ for a in pipeline.analyses] == ["Hmm", "GlobalCoverage", "LocalCoverage", "Substitutions", "Indels", "AlignmentUncertainty",
                                                       "ChannelMappability", "KmerAnalysis", "IndelKmerAnalysis"]
    assert [m.__name__ for m in pipeline.metaAnalyses] == ["UnmappedKmerAnalysis", "CoverageSummary", "UnmappedLengthDistributionAnalysis",
                                                           "ComparePerReadMappabilityByMapper", "HmmMetaAnalysis", "CoverageDepth"]
    assert pipeline.resolveClasses("SeedMapperChain, LastParamsRealignEm", "nanopore_amd.mappers", AbstractMapper) == [variants.SeedMapperChain, variants.LastParamsRealignEm]
    assert pipeline.resolveClasses("Hmm,GlobalCoverage", "nanopore_amd.analyses", AbstractAnalysis) == [HmmAnalysis, GlobalCoverage]
    assert pipeline.resolveClasses("CoverageDepth,CoverageSummary", "nanopore_amd.metaAnalyses", AbstractMetaAnalysis) == [CoverageDepth, CoverageSummary]
    with pytest.raises(RuntimeError, match="NoSuchMapper"):
        pipeline.resolveClasses("NoSuchMapper", "nanopore_amd.mappers", AbstractMapper)
    with pytest.raises(RuntimeError, match="SeedMapperChain"):   # a mapper is no analysis
        pipeline.resolveClasses("SeedMapperChain", "nanopore_amd.analyses", AbstractAnalysis)


# ---- unique names ----

def test_fastq_names_made_unique(tmp_path):
    """The suffix form: `<name>_<k>`, k the smallest number from 1 that gives a name not taken yet."""
    records = [(b"a x", b"ACGTacgtNN", b"!!##IIii~~"), (b"a y", b"TTTT", b"@@@@"), (b"b", b"G", b"+"), (b"a", b"CCCCC", b"IIIII"),
               (b"a_1\tz", b"AC", b"II"), (b"b", b"T", b"@")]
    src, dst = str(tmp_path / "in.fq"), str(tmp_path / "out.fq")
    with open(src, "wb") as fh:
        for name, seq, qual in records:
            fh.write(b"@" + name + b"\n" + seq + b"\n+" + b"\n" + qual + b"\n")
    assert makeFastqSequenceNamesUnique(src, dst) == dst
    lines = open(dst, "rb").read().split(b"\n")
    assert lines[-1] == b"" and len(lines) == 4 * len(records) + 1
    assert lines[0:-1:4] == [b"@a", b"@a_1", b"@b", b"@a_2", b"@a_1_1", b"@b_1"]
    assert lines[1:-1:4] == [r[1] for r in records] and lines[3:-1:4] == [r[2] for r in records]   # sequence and quality bytes as they were
    assert lines[2:-1:4] == [b"+"] * len(records)
    assert open(src, "rb").read().split(b"\n")[0] == b"@a x"                                        # the input is left alone


def test_fasta_names_made_unique(tmp_path):
    src, dst = str(tmp_path / "in.fa"), str(tmp_path / "out.fa")
    text = b">a x\nACGTAC\nacgtnn\nGG\n>a y\nTTTT\n>b\nG\n>a\nCC\nCCC\n"
    with open(src, "wb") as fh:
        fh.write(text)
    assert makeFastaSequenceNamesUnique(src, dst) == dst
    assert open(dst, "rb").read() == b">a\nACGTAC\nacgtnn\nGG\n>a_1\nTTTT\n>b\nG\n>a_2\nCC\nCCC\n"   # multi-line sequences keep their lines
    from nanopore_amd import ingest
    assert ingest.FastaTable(dst).names == ["a", "a_1", "b", "a_2"]                                  # (the duplicate-name assert does not fire)


# ---- Hmm and HmmMetaAnalysis ----

def _trial_models(seed):
    """Three trial models with transitions on the used pairs only (so some avgs are 0) and their running likelihoods."""
    rng = np.random.default_rng(seed)
    models, running = [], []
    for trial in range(3):
        h = em.randomise(Hmm(), rng)
        h.likelihood = -1000.0 - 10 * trial - seed
        models.append(h)
        running.append([-2000.0 + 100.5 * i - trial for i in range(4 + trial)])
    return models, running


def _tsv(path):
    rows = [ln.split("\t") for ln in open(path).read().split("\n")[:-1]]
    return rows[0], rows[1:]


def _dot_edges(path):
    """{(from, to): label} of a DOT file, after checking that it is a graph of the five named states."""
    text = open(path).read()
    lines = text.split("\n")
    assert lines[0] == "graph G {" and lines[-2:] == ["}", ""]
    nodes = dict(re.findall(r'^(n\dn) \[label="([a-z ]+)"', text, flags=re.M))
    assert nodes == {"n0n": "match", "n1n": "short delete", "n2n": "short insert", "n3n": "long insert", "n4n": "long delete"}
    edges = re.findall(r'^n(\d)n -- n(\d)n \[label="([^"]*)".*\];$', text, flags=re.M)
    assert len(edges) == sum(" -- " in ln for ln in lines) and all(ln.endswith(";") for ln in lines[1:-2])
    out = {(a, b): label for a, b, label in edges}
    assert len(out) == len(edges)
    return out


def test_hmm_analysis_tables_and_graph(tmp_path):
    models, running = _trial_models(3)
    exp = tmp_path / "experiment"
    out = exp / "analysis_Hmm"
    out.mkdir(parents=True)
    em.writeXML(str(exp / "hmm.txt.xml"), models, running)
    an = HmmAnalysis("reads.fq", "2D", "ref.fa", str(exp / "mapping.sam"), str(out))
    an.run()
    an.cleanup()
    assert sorted(os.listdir(str(out))) == ["DONE", "hmm.dot", "indelEmissions.tsv", "matchEmissions.tsv", "runninglikelihoods.tsv"]
    T = np.array([m.transitions for m in models]).reshape(3, 5, 5)
    E = np.array([m.emissions for m in models]).reshape(3, 5, 4, 4)   # trial, state, x, y
    # matchEmissions: the XML's strings, which are str() of the mean over the trials
    header, rows = _tsv(str(out / "matchEmissions.tsv"))
    assert header == list(BASES) and [r[0] for r in rows] == list(BASES)
    xml = {(e.get("state"), e.get("x"), e.get("y")): e.get("avg") for e in ET.parse(str(exp / "hmm.txt.xml")).getroot().findall("emission")}
    for i, x in enumerate(BASES):
        for j, y in enumerate(BASES):
            assert rows[i][1 + j] == xml["0", x, y] == str(float(E[:, 0, i, j].mean()))
    # indelEmissions: insert row = state 2 summed over y per x, delete row = state 1 summed over x per y
    header, rows = _tsv(str(out / "indelEmissions.tsv"))
    assert header == list(BASES) and len(rows) == 2
    for i in range(4):
        assert float(rows[0][i]) == pytest.approx(E[:, 2, i, :].mean(axis=0).sum(), rel=1e-12)
        assert float(rows[1][i]) == pytest.approx(E[:, 1, :, i].mean(axis=0).sum(), rel=1e-12)
    # runninglikelihoods: a line per trial
    lines = open(str(out / "runninglikelihoods.tsv")).read().split("\n")
    assert lines[-1] == "" and len(lines) == 4
    for line, want in zip(lines, running):
        assert [float(v) for v in line.split("\t")] == want
    # the graph: an edge per transition whose mean is above 0 -- the fifteen used ones
    edges = _dot_edges(str(out / "hmm.dot"))
    assert set(edges) == {(str(a), str(b)) for a, b in em.USED_TRANSITIONS} and len(edges) == 15
    for (a, b), label in edges.items():
        assert label == "%.3f,%.3f" % (T[:, int(a), int(b)].mean(), T[:, int(a), int(b)].std())


def test_hmm_analysis_without_a_model_only_finishes(tmp_path):
    exp = tmp_path / "experiment"
    out = exp / "analysis_Hmm"
    out.mkdir(parents=True)
    an = HmmAnalysis("reads.fq", "2D", "ref.fa", str(exp / "mapping.sam"), str(out))
    an.run()
    an.cleanup()
    assert os.listdir(str(out)) == ["DONE"] and AbstractAnalysis.isFinished(str(out))


def test_hmm_meta_analysis_averages_over_experiments(tmp_path):
    class SeedMapperRealignEm(object):
        pass

    class SeedMapperChain(object):
        pass

    a, b = _trial_models(3), _trial_models(8)
    b[0][1].transitions[0 * 5 + 4] = b[0][0].transitions[0 * 5 + 4] = b[0][2].transitions[0 * 5 + 4] = 0.0   # an edge only one experiment has
    experiments = []
    for k, (readType, mapper, model) in enumerate((("2D", SeedMapperRealignEm, a), ("2D", SeedMapperChain, None), ("2D", SeedMapperRealignEm, b),
                                                   ("template", SeedMapperRealignEm, None))):
        d = tmp_path / ("experiment_%d" % k)
        d.mkdir()
        if model is not None:
            em.writeXML(str(d / "hmm.txt.xml"), *model)
        experiments.append(("reads%d.fq" % (k // 2), readType, "ref.fa", mapper, [], str(d)))
    out = tmp_path / "metaAnalysis_HmmMetaAnalysis"
    out.mkdir()
    m = HmmMetaAnalysis(str(out), experiments)
    m.run()
    m.cleanup()
    # the read type without any model writes nothing
    assert sorted(os.listdir(str(out))) == ["hmm_2D.dot", "matchEmissionsNormalisedByReference_2D.tsv", "matchEmissionsUnnormalisedStdErrors_2D.tsv",
                                            "matchEmissionsUnnormalised_2D.tsv"]
    # per experiment what its XML holds: mean and std over its three trials; then the mean over the two experiments
    Ts = [np.array([h.transitions for h in model[0]]).reshape(3, 5, 5).mean(axis=0) for model in (a, b)]
    Es = [np.array([h.emissions for h in model[0]]).reshape(3, 5, 4, 4)[:, 0] for model in (a, b)]
    avg = np.mean([e.mean(axis=0) for e in Es], axis=0)
    std = np.mean([e.std(axis=0) for e in Es], axis=0)
    for name, want in (("matchEmissionsUnnormalised", avg), ("matchEmissionsUnnormalisedStdErrors", std),
                       ("matchEmissionsNormalisedByReference", avg / avg.sum(axis=1, keepdims=True))):
        header, rows = _tsv(str(out / (name + "_2D.tsv")))
        assert header == list(BASES) and [r[0] for r in rows] == list(BASES)
        got = np.array([[float(v) for v in r[1:]] for r in rows])
        assert got.shape == (4, 4) and np.allclose(got, want, rtol=1e-12, atol=0)
    assert not np.allclose(avg, Es[0].mean(axis=0), rtol=1e-3)   # (not the first experiment's numbers)
    edges = _dot_edges(str(out / "hmm_2D.dot"))
    assert set(edges) == {(str(x), str(y)) for x, y in em.USED_TRANSITIONS}
    for (x, y), label in edges.items():
        values = [T[int(x), int(y)] for T in Ts if T[int(x), int(y)] > 0]
        assert len(values) == (1 if (x, y) == ("0", "4") else 2)
        assert label == "%.3f,%.3f" % (np.mean(values), np.std(values))


# ---- ChannelMappability ----

def _channel_files(tmp_path, records):
    seq = "ACGTACGTAC"
    names = ["channel_1_read_3", "channel_1_read_12 2D", "channel_7_read_1", "channel_600_read_0", "channel_600_read_5_twodirections", "not_a_channel_1_read_1"]
    fq, sam = str(tmp_path / "reads.fq"), str(tmp_path / "mapping.sam")
    with open(fq, "w") as fh:
        for n in names:
            fh.write("@%s\n%s\n+\n%s\n" % (n, seq, "I" * len(seq)))
    with open(sam, "w") as fh:
        fh.write("@SQ\tSN:ref\tLN:100\n")
        for name, flag, rname in records:
            fh.write("\t".join([name, str(flag), rname, "1" if rname != "*" else "0", "255", "10M" if rname != "*" else "*", "*", "0", "0", seq, "*"]) + "\n")
    out = tmp_path / "analysis_ChannelMappability"
    out.mkdir()
    an = ChannelMappability(fq, "2D", "ref.fa", sam, str(out))
    an.run()
    an.cleanup()
    assert AbstractAnalysis.isFinished(str(out))
    return str(out / "channel_mappability.tsv")


def test_channel_mappability_counts_records_per_channel(tmp_path):
    # two records of one channel-1 read, one of a channel-600 read, channel 7 with the unmapped flag, one of a name that is no channel name
    path = _channel_files(tmp_path, [("channel_1_read_12", 0, "ref"), ("channel_1_read_12", 16, "ref"), ("channel_600_read_0", 0, "ref"),
                                     ("channel_7_read_1", 4, "ref"), ("not_a_channel_1_read_1", 0, "ref")])
    lines = open(path).read().split("\n")
    assert lines[0] == "Channel\tReadCount\tMappableReadCount" and lines[-1] == ""
    rows = [tuple(int(v) for v in ln.split("\t")) for ln in lines[1:-1]]
    assert len(rows) == max(513, 600) - 1 == 599
    want = {1: (2, 2), 7: (1, 0)}             # (channel 600 is the row the reference's range leaves out)
    assert rows == [(c,) + want.get(c, (0, 0)) for c in range(1, 600)]


def test_channel_mappability_writes_nothing_without_mapped_channel_reads(tmp_path):
    path = _channel_files(tmp_path, [("channel_7_read_1", 4, "ref"), ("channel_1_read_3", 4, "*"), ("not_a_channel_1_read_1", 0, "ref")])
    assert not os.path.exists(path)
    assert os.listdir(os.path.dirname(path)) == ["DONE"]


# ---- CoverageSummary ----

ATTRS = ("avgreadCoverage", "avgreferenceCoverage", "avgidentity", "avgmismatchesPerReadBase", "avgdeletionsPerReadBase", "avginsertionsPerReadBase",
         "numberOfMappedReads", "numberOfUnmappedReads", "numberOfReads")


def _coverage_experiment(root, k, readFile, mapper, with_xml=True):
    """An experiment directory with a hand-written coverage_bestPerRead.xml whose strings are the experiment's own."""
    d = os.path.join(str(root), "experiment_%d" % k, "analysis_GlobalCoverage")
    os.makedirs(d)
    values = ["0.%d%d25" % (k, i) for i in range(6)] + [str(10 + k), str(k), str(10 + 2 * k)]
    attrib = dict(zip(ATTRS, values), distributionidentity=" ".join("0.%d%d" % (k, j) for j in range(2 + k)), avgreadLength="nan")
    if with_xml:
        with open(os.path.join(d, "coverage_bestPerRead.xml"), "w") as fh:
            fh.write(ET.tostring(ET.Element("coverage_bestPerRead", attrib)).decode())
    return (os.path.join("/data/processed", readFile), "2D", "/data/refs/ref.fa", mapper, [], os.path.dirname(d)), values, attrib["distributionidentity"].split()


def test_coverage_summary_tables(tmp_path):
    class SeedMapperChain(object):
        pass

    class SeedMapperRealign(object):
        pass

    out = tmp_path / "metaAnalysis_CoverageSummary"
    out.mkdir()
    made = [_coverage_experiment(tmp_path, 1, "readsA.fq", SeedMapperChain), _coverage_experiment(tmp_path, 2, "readsA.fq", SeedMapperRealign),
            _coverage_experiment(tmp_path, 3, "readsB.fq", SeedMapperRealign), _coverage_experiment(tmp_path, 4, "readsB.fq", SeedMapperChain, with_xml=False)]
    m = CoverageSummary(str(out), [e for e, _, _ in made])
    m.run()
    m.cleanup()
    assert len(m.db) == 3
    tables = {"Seed_2D_ref.fa", "Seed_readsA.fq", "Seed_readsB.fq", "ref.fa"}
    assert set(os.listdir(str(out))) == {t + ".csv" for t in tables} | {t + "_distribution.csv" for t in tables}

    def row(k, name):
        e, values, _ = made[k - 1]
        return [name, e[3].__name__, "2D", os.path.basename(e[0]), "ref.fa"] + values

    want = {"Seed_2D_ref.fa": [row(1, "SeedMapperChain"), row(2, "SeedMapperRealign"), row(3, "SeedMapperRealign.2")],
            "Seed_readsA.fq": [row(1, "SeedMapperChain"), row(2, "SeedMapperRealign")],
            "Seed_readsB.fq": [row(3, "SeedMapperRealign")],
            "ref.fa": [row(1, "SeedMapperChain_2D"), row(2, "SeedMapperRealign_2D"), row(3, "SeedMapperRealign_2D.2")]}
    for t, rows in want.items():
        lines = open(str(out / (t + ".csv"))).read().split("\n")
        assert lines[0] == ",".join(COLUMNS) == ("Name,Mapper,ReadType,ReadFile,ReferenceFile,AvgReadCoverage,AvgReferenceCoverage,AvgIdentity,AvgMismatchesPerReadBase,"
                                                 "AvgDeletionsPerReadBase,AvgInsertionsPerReadBase,NumberOfMappedReads,NumberOfUnmappedReads,NumberOfReads")
        assert [ln.split(",") for ln in lines[1:-1]] == rows and lines[-1] == ""
        dist = open(str(out / (t + "_distribution.csv"))).read().split("\n")
        assert [ln.split(",") for ln in dist[:-1]] == [[r[0]] + made[int(r[5][2]) - 1][2] for r in rows] and dist[-1] == ""


def test_coverage_summary_duplicate_row_names():
    from nanopore_amd.metaAnalyses.coverageSummary import Entry

    def entries(*pairs):
        return [Entry(readType, "reads.fq", "ref.fa", type(mapper, (object,), {}), None) for mapper, readType in pairs]

    m = CoverageSummary("/nowhere", [])
    m.cleanup()
    es = entries(("A", "2D"), ("A", "2D"), ("A", "template"), ("B", "2D"), ("B", "2D"), ("B", "2D"))
    assert m.resolve_duplicate_rownames(es) == ["A", "A.2", "A.3", "B", "B.2", "B.3"]
    assert m.resolve_duplicate_rownames(es, multiple_read_types=True) == ["A_2D", "A_2D.2", "A_template", "B_2D", "B_2D.2", "B_2D.3"]
    m.write_file_analyze([], "empty")   # a grouping without entries: no file, no error
