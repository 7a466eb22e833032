"""The pipeline driver end to end on the device: tests/golden/c1 (two reads of 32 750 and 38 435 bases, one reference of 57.5 kb)
as a working directory with one read type, through `pipeline.main`.

SeedMapper's defaults (k 16, minLength 20) map both reads -- 115 maximal exact matches of 20 bases or more for the first read
on the forward strand, 204 for the second on the reverse strand, counted on the host with tests/seed_reference.py
(DictionaryOracle(reference, 16).matches(read, 20)) -- so no subclass with a lower minLength is needed, and two reads need no
subsampling.  The fixture's names (MOUSE_1_read_1, RAT_1_read_1) are no channel names, and ChannelMappability would have nothing
to write; the working directory's copy therefore gives the first read the header `channel_12_read_1 MOUSE_1_read_1` (bases and
qualities as they are) and leaves the second as it is: one of the two mapped records counts, the other must not.
"""
import os
import re
import time
import xml.etree.ElementTree as ET

import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu

C1 = os.path.join(ROOT, "tests", "golden", "c1")


def _working_dir(root):
    reads = os.path.join(str(root), "readFastqFiles", "2D")
    refs = os.path.join(str(root), "referenceFastaFiles")
    os.makedirs(reads)
    os.makedirs(refs)
    lines = open(os.path.join(C1, "reads.fq"), "rb").read().split(b"\n")
    assert lines[0] == b"@MOUSE_1_read_1" and lines[4] == b"@RAT_1_read_1"
    lines[0] = b"@channel_12_read_1 MOUSE_1_read_1"
    with open(os.path.join(reads, "reads.fq"), "wb") as fh:
        fh.write(b"\n".join(lines))
    with open(os.path.join(refs, "reference.fa"), "wb") as fh:
        fh.write(open(os.path.join(C1, "reference.fa"), "rb").read())
    return str(root)


def _processed(work):
    return (os.path.join(work, "output", "processedReadFastqFiles", "2D", "reads.fq"),
            os.path.join(work, "output", "processedReferenceFastaFiles", "reference.fa"))


def _experiment(work, mapper):
    return os.path.join(work, "output", "analysis_2D", "experiment_reads.fq_reference.fa_" + mapper)


def test_driver_on_c1_chain_and_realign(tmp_path):
    from nanopore_amd import pipeline
    from nanopore_amd.analyses.abstractAnalysis import AbstractAnalysis
    from nanopore_amd.mappers import variants
    work = _working_dir(tmp_path / "work")
    names = ("SeedMapperChain", "SeedMapperRealign")
    t0 = time.perf_counter()
    assert pipeline.main([work, "--mappers", ",".join(names)]) == 0
    print("pipeline.main on c1, %s, default analyses and meta-analyses: %.2f s" % (" + ".join(names), time.perf_counter() - t0))
    fq, fa = _processed(work)
    assert open(fq, "rb").read().split(b"\n")[0:5:4] == [b"@channel_12_read_1", b"@RAT_1_read_1"] and open(fa, "rb").readline() == b">HUMAN\n"
    assert sorted(os.listdir(os.path.join(work, "output", "analysis_2D"))) == [os.path.basename(_experiment(work, n)) for n in names]

    for name in names:
        exp = _experiment(work, name)
        # SAM identity: the mapper class on its own, on the processed files
        direct = str(tmp_path / (name + ".sam"))
        mapper = getattr(variants, name)(fq, "2D", fa, direct, str(tmp_path / (name + ".hmm.txt")))
        mapper.run()
        mapper.cleanup()
        sam = open(os.path.join(exp, "mapping.sam"), "rb").read()
        assert sam == open(direct, "rb").read()
        records = [ln.split(b"\t") for ln in sam.split(b"\n") if ln and not ln.startswith(b"@")]
        assert sorted(r[0] for r in records) == [b"RAT_1_read_1", b"channel_12_read_1"]            # both reads map, one record each
        # analysis completion
        assert sorted(os.listdir(exp)) == sorted(["mapping.sam"] + ["analysis_" + a.__name__ for a in pipeline.analyses])
        for a in pipeline.analyses:
            assert AbstractAnalysis.isFinished(os.path.join(exp, "analysis_" + a.__name__)), a.__name__
        assert os.listdir(os.path.join(exp, "analysis_Hmm")) == ["DONE"]                              # no model was trained
        # channel total: the mapped column against a scan of the records made here
        mapped = sum(1 for r in records if not int(r[1]) & 4 and r[2] != b"*" and re.match(br"channel_[0-9]+_read_[0-9]+", r[0]))
        rows = [ln.split("\t") for ln in open(os.path.join(exp, "analysis_ChannelMappability", "channel_mappability.tsv")).read().split("\n")[1:-1]]
        assert len(rows) == 512 and sum(int(r[2]) for r in rows) == mapped == 1
        assert [r for r in rows if r[1:] != ["0", "0"]] == [["12", "1", "1"]]

    # CSV versus XML: the CoverageSummary row of each mapper repeats its experiment's coverage_bestPerRead.xml
    meta = os.path.join(work, "output", "metaAnalysis_CoverageSummary")
    for table in ("Seed_2D_reference.fa", "Seed_reads.fq", "reference.fa"):
        lines = open(os.path.join(meta, table + ".csv")).read().split("\n")
        assert len(lines) == 4 and lines[-1] == ""
        for line, name in zip(lines[1:3], names):
            root = ET.parse(os.path.join(_experiment(work, name), "analysis_GlobalCoverage", "coverage_bestPerRead.xml")).getroot()
            assert root.get("numberOfMappedReads") == "2" and root.get("numberOfReads") == "2"
            assert line.split(",") == [name + ("_2D" if table == "reference.fa" else ""), name, "2D", "reads.fq", "reference.fa"] + [
                root.attrib[k] for k in ("avgreadCoverage", "avgreferenceCoverage", "avgidentity", "avgmismatchesPerReadBase", "avgdeletionsPerReadBase",
                                         "avginsertionsPerReadBase", "numberOfMappedReads", "numberOfUnmappedReads", "numberOfReads")]
        dist = open(os.path.join(meta, table + "_distribution.csv")).read().split("\n")
        assert [len(ln.split(",")) for ln in dist[:-1]] == [3, 3]
    # the other meta-analyses ran on the same experiments
    out = os.path.join(work, "output")
    assert sorted(d for d in os.listdir(out) if d.startswith("metaAnalysis_")) == sorted("metaAnalysis_" + m.__name__ for m in pipeline.metaAnalyses)
    assert os.listdir(os.path.join(out, "metaAnalysis_HmmMetaAnalysis")) == []
    for name in names:
        assert os.path.getsize(os.path.join(out, "metaAnalysis_CoverageDepth", os.path.basename(_experiment(work, name)) + "_Depth.txt")) > 0
    assert open(os.path.join(out, "metaAnalysis_ComparePerReadMappabilityByMapper", "2D_perReadMappability.tsv")).read() == \
        "Read\tReadFastqFile\tSeed\nchannel_12_read_1\treads.fq\t1\nRAT_1_read_1\treads.fq\t1\n"


def test_driver_on_c1_realign_em_trains_and_draws_the_model(tmp_path, monkeypatch):
    from nanopore_amd import em, pipeline
    Options = em.Options

    class ShortOptions(Options):
        """The trainer's defaults (utils.learnModelFromSamFileTargetFn takes em.Options()) with two iterations instead of a hundred."""

        def __init__(self):
            Options.__init__(self)
            self.iterations, self.seed = 2, 11

    monkeypatch.setattr(em, "Options", ShortOptions)
    trials = ShortOptions().trials
    assert trials == 3
    work = _working_dir(tmp_path / "work")
    t0 = time.perf_counter()
    assert pipeline.main([work, "--mappers", "SeedMapperRealignEm", "--analyses", "Hmm", "--metaAnalyses", "HmmMetaAnalysis"]) == 0
    print("pipeline.main on c1, SeedMapperRealignEm (%d trials of %d iterations), Hmm, HmmMetaAnalysis: %.2f s" % (trials, 2, time.perf_counter() - t0))
    exp = _experiment(work, "SeedMapperRealignEm")
    assert os.path.isfile(os.path.join(exp, "hmm.txt.xml")) and os.path.isfile(os.path.join(exp, "hmm.txt")) and os.path.getsize(os.path.join(exp, "mapping.sam")) > 70000
    out = os.path.join(exp, "analysis_Hmm")
    assert sorted(os.listdir(out)) == ["DONE", "hmm.dot", "indelEmissions.tsv", "matchEmissions.tsv", "runninglikelihoods.tsv"]
    lines = open(os.path.join(out, "runninglikelihoods.tsv")).read().split("\n")
    assert len(lines) == trials + 1 and lines[-1] == ""
    for line in lines[:-1]:
        values = [float(v) for v in line.split("\t")]
        assert len(values) == 2 + 1 and values[1] > values[0]           # before each update and after the last; EM does not lose likelihood
    root = ET.parse(os.path.join(exp, "hmm.txt.xml")).getroot()
    rows = [ln.split("\t") for ln in open(os.path.join(out, "matchEmissions.tsv")).read().split("\n")[1:-1]]
    assert [r[0] for r in rows] == list("ACGT")
    assert [v for r in rows for v in r[1:]] == [e.get("avg") for e in root.findall("emission") if e.get("state") == "0"]
    assert open(os.path.join(out, "hmm.dot")).read().count(" -- ") == sum(float(t.get("avg")) > 0 for t in root.findall("transition")) >= 13
    assert sorted(os.listdir(os.path.join(work, "output", "metaAnalysis_HmmMetaAnalysis"))) == [
        "hmm_2D.dot", "matchEmissionsNormalisedByReference_2D.tsv", "matchEmissionsUnnormalisedStdErrors_2D.tsv", "matchEmissionsUnnormalised_2D.tsv"]
