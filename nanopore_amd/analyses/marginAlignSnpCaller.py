"""MarginAlignSnpCaller: SNP calling from posterior match probabilities marginalised over alignments
(nanopore/analyses/marginAlignSnpCaller.py:14-308).

The reference runs `cactus_realign --outputAllPosteriorProbs` once per read, hmm type, coverage and replicate
(:135-146) and adds every `refPos readPos prob` line into per-position base expectations (:149-155).  A read's
posteriors do not depend on which other reads are sampled, so here each hmm type costs ONE batched GPU call
(NPR_MODE_ALL_POSTERIORS, --splitMatrixBiggerThanThis=100) over all reads; the coverage / replicate loops only
re-sample which reads' posteriors are accumulated.  Output: marginaliseConsensus.xml with the reference's element
and attribute names (:268-303).

The calling itself -- candidate posteriors per position, one call per non-reference base, the curves over 101
thresholds -- runs on the host by default; `MarginAlignSnpCaller.callsOnDevice = True` makes and counts the calls on the
device (csrc/npr_snpcall.hip) and writes the same file.  The held-out SNPs come from analyses/mutate_reference.py.
"""
import math
import os
import random
import xml.etree.ElementTree as ET
from itertools import product

import numpy as np

from .. import sam as pysam
from ..hmm import Hmm
from .abstractAnalysis import AbstractAnalysis
from .alignmentUncertainty import prettyXml
from .utils import (ANALYSIS_SPLIT_MATRIX_BIGGER_THAN, alignedPairs, getFastaDictionary, getFastqDictionary,
                    realignRecords, samIterator, trainedModelPath)

bases = "ACGT"
_BASE_CODE = np.full(256, -1, dtype=np.int64)
for _k, _c in enumerate(bases):
    _BASE_CODE[ord(_c)] = _BASE_CODE[ord(_c.lower())] = _k


# ---- substitution models: 4 x 4 arrays [from, to] over ACGT; the dict forms keep the reference's function names ----

def errorMatrixOfHmm(hmmFile):
    """P(observed base | true base) from a model's match emissions: the 4 x 4 block, every row scaled to sum 1
    (marginAlignSnpCaller.py:25-29)."""
    block = np.asarray(Hmm.loadHmm(hmmFile).emissions[:16], dtype=np.float64).reshape(4, 4)
    return block / block.sum(axis=1, keepdims=True)


NULL_MATRIX = np.ones((4, 4))                                      # no evolutionary prior (:31-32)
FLAT_ERROR_MATRIX = np.where(np.eye(4, dtype=bool), 0.8, 0.2 / 3)  # Jukes-Cantor-like (:34-35)


def _asDict(matrix):
    return {(bases[i], bases[j]): float(matrix[i, j]) for i in range(4) for j in range(4)}


def loadHmmErrorSubstitutionMatrix(hmmFile):
    return _asDict(errorMatrixOfHmm(hmmFile))


def getNullSubstitutionMatrix():
    return _asDict(NULL_MATRIX)


def getJukesCantorTypeSubstitutionMatrix():
    return _asDict(FLAT_ERROR_MATRIX)


def getProb(subMatrix, start, end):
    return subMatrix[(start, end)]


def basePosteriors(observed, refCodes, evolutionMatrix, errorMatrix):
    """Posterior of each candidate true base at many positions at once (:18-23, vectorised): observed[p, o] = fraction of
    the position's evidence that says base o, refCodes[p] = the reference base there.
    log P(candidate c) = log evolution[ref, c] + sum_o observed[o] * log error[c, o], normalised over c."""
    with np.errstate(divide="ignore"):
        logp = np.log(evolutionMatrix)[refCodes] + observed @ np.log(errorMatrix).T
    logp -= logp.max(axis=1, keepdims=True)
    w = np.exp(logp)
    return w / w.sum(axis=1, keepdims=True)


def calcBasePosteriorProbs(baseObservations, refBase, evolutionarySubstitionMatrix, errorSubstutionMatrix):
    """The one-position dict form of basePosteriors (the reference's signature)."""
    toArray = lambda d: np.array([[d[(a, b)] for b in bases] for a in bases], dtype=np.float64)  # noqa: E731
    post = basePosteriors(np.array([[baseObservations[b] for b in bases]], dtype=np.float64), np.array([bases.index(refBase)]),
                          toArray(evolutionarySubstitionMatrix), toArray(errorSubstutionMatrix))[0]
    return dict(zip(bases, post.tolist()))


class SnpCalls(object):
    """A set of SNP calls, each with the posterior probability it was made with, and its precision / recall curves over the
    101 probability thresholds 0.00 .. 1.00 (:163-197): a call counts at every threshold up to its (rounded) probability."""

    def __init__(self, totalHeldOut):
        self.totalHeldOut = totalHeldOut
        self.truePositives = []   # (probability, reference position)
        self.falsePositives = []
        self.falseNegatives = []
        self.notCalled = 0
        self.histograms = None    # fromHistograms: (true positives, false positives) per round(100 p), instead of the two lists

    @classmethod
    def fromHistograms(cls, totalHeldOut, true_pos, false_pos, notCalled):
        """The same curves from calls that were counted where they were made (Batch.snp_calls, Pileup.snp_calls): true_pos[b] / false_pos[b] =
        number of true / false calls with round(100 p) == b, b = 0..100.  No list of calls exists."""
        calls = cls(totalHeldOut)
        calls.histograms = (np.asarray(true_pos, dtype=np.float64).reshape(101), np.asarray(false_pos, dtype=np.float64).reshape(101))
        calls.notCalled = int(notCalled)
        return calls

    @staticmethod
    def cumulate(hist):
        """[sum of hist[t:] for t in 0..100], as floats: what bucket() makes of the calls the histogram counts."""
        return np.asarray(hist, dtype=np.float64)[::-1].cumsum()[::-1].tolist()

    @staticmethod
    def bucket(calls):
        """[number of calls with round(100 p) >= t for t in 0..100], as floats."""
        p = np.asarray(list(calls), dtype=np.float64)
        hist = np.bincount(np.rint(p * 100).astype(np.int64), minlength=101).astype(np.float64) if len(p) else np.zeros(101)
        return hist[::-1].cumsum()[::-1].tolist()

    def _bucketed(self, true):
        if self.histograms is not None:
            return self.cumulate(self.histograms[0 if true else 1])
        return self.bucket(p for p, _ in (self.truePositives if true else self.falsePositives))

    def addCalls(self, probabilities, positions, isTrue):
        for p, x, t in zip(probabilities.tolist(), positions.tolist(), isTrue.tolist()):
            (self.truePositives if t else self.falsePositives).append((p, x))

    def getPrecisionByProbability(self):
        tp = np.array(self._bucketed(True))
        fp = np.array(self._bucketed(False))
        made = tp + fp
        return [float(t / m) if m else 0 for t, m in zip(tp, made)]

    def getRecallByProbability(self):
        return [t / self.totalHeldOut if self.totalHeldOut else 0 for t in self._bucketed(True)]


def loadHeldOutSnps(referenceFastaFile, refSequences):
    """The truth behind a mutated reference: `<reference>_Index.txt` holds every sequence twice, as it was and (name +
    "_mutated") as the reference FASTA has it (written by mutate_reference.py; read at :60-78).  Returns
    {(sequence name, position): true base} for every position where the two differ; {} when there is no such file."""
    truthFile = referenceFastaFile + "_Index.txt"
    if not os.path.exists(truthFile):
        return {}
    pairs = getFastaDictionary(truthFile)
    originals = [n for n in pairs if n in refSequences]
    strays = [n for n in pairs if n not in refSequences and not n.endswith("_mutated")]
    assert not strays, "unexpected sequences in %s: %s" % (truthFile, strays)
    assert len(originals) == len(refSequences), "%s does not cover the reference" % truthFile
    held = {}
    for name in originals:
        true, mutated = pairs[name], pairs[name + "_mutated"]
        assert mutated == refSequences[name], "%s_mutated is not the reference sequence" % name
        a = np.frombuffer(true.encode(), dtype=np.uint8)
        b = np.frombuffer(mutated.encode(), dtype=np.uint8)
        for i in np.flatnonzero(a != b).tolist():
            held[(name, i)] = true[i]
    return held


class MarginAlignSnpCaller(AbstractAnalysis):
    hmmTypes = ("cactus", "trained_0", "trained_20", "trained_40")
    coverages = (1000000, 120, 60, 30, 10)
    # True: the calls of every sample are made and counted on the device (Batch.snp_calls on the posterior expectations where they lie,
    # Pileup.snp_calls on a pileup of the sampled records); no [positions][4] table crosses PCIe and no list of calls exists on the host.
    # Same XML.  Off until the two paths have been timed on hardware (tools/snp_calls_time.py).
    callsOnDevice = False

    def run(self, ctx=None, seed=None):
        from .. import realign
        AbstractAnalysis.run(self)
        rng = random.Random(seed)
        refSequences = getFastaDictionary(self.referenceFastaFile)
        readSequences = getFastqDictionary(self.readFastqFile)
        refNames = sorted(refSequences)
        refIndex = {n: i for i, n in enumerate(refNames)}
        totalReferenceLength = sum(len(s) for s in refSequences.values())
        snpSet = loadHeldOutSnps(self.referenceFastaFile, refSequences)
        hmmErrorMatrix = errorMatrixOfHmm(trainedModelPath("blasr_hmm_20.txt"))  # :56
        hmmFiles = {"cactus": None, "trained_0": trainedModelPath("blasr_hmm_0.txt"),
                    "trained_20": trainedModelPath("blasr_hmm_20.txt"), "trained_40": trainedModelPath("blasr_hmm_40.txt")}
        sam = pysam.Samfile(self.samFile, "r")
        records = list(samIterator(sam))
        for aR in records:  # :127-130
            refSeq = refSequences[sam.getrname(aR.rname)]
            assert aR.pos == 0 and aR.qstart == 0 and aR.qend == len(aR.query) and aR.aend == len(refSeq)
        # frequencies of aligned bases per read, from the SAM alignment itself (:111-118)
        alignedBases = []
        for aR in ([] if self.callsOnDevice else records):  # (callsOnDevice: a pileup of the records on the device instead)
            refName = sam.getrname(aR.rname)
            pos, code = [], []
            query = aR.query.upper()
            for r, q in alignedPairs(aR, len(refSequences[refName])):
                pos.append(r)
                code.append(bases.find(query[q]))
            alignedBases.append((refIndex[refName], np.array(pos, dtype=np.int64), np.array(code, dtype=np.int64)))
        staged = self._stageForDevice(sam, records, refSequences, refNames, refIndex, snpSet) if self.callsOnDevice else None
        node = ET.Element("marginAlignComparison")
        for hmmType in self.hmmTypes:
            # one batched GPU call per hmm type: all posterior match probabilities of every read (:135-146).  The pairs
            # stay in HBM: each coverage sample below scatter-adds them per reference position on the device
            # (npr_batch_base_expectations) instead of parsing a `refPos readPos prob` file per read (:149-155).
            from .utils import _context, _loadHmmInto, stageSamFile
            ctx = ctx or _context()
            _loadHmmInto(ctx, hmmFiles[hmmType])
            batch, stagedSam, _ = stageSamFile(self.samFile, self.referenceFastaFile, ANALYSIS_SPLIT_MATRIX_BIGGER_THAN,
                                               mode=realign.MODE_ALL_POSTERIORS, ctx=ctx, maxPairsPerBase=48)
            stagedSam.close()
            try:
                self._callsOfOneModel(node, hmmType, batch, records, refSequences, readSequences, refNames, alignedBases, snpSet,
                                      hmmErrorMatrix, totalReferenceLength, rng, staged)
            finally:
                batch.close()
        sam.close()
        with open(os.path.join(self.outputDir, "marginaliseConsensus.xml"), "w") as fh:
            fh.write(prettyXml(node))
        self.finish()
        return node

    @staticmethod
    def _stageForDevice(sam, records, refSequences, refNames, refIndex, snpSet):
        """What callsOnDevice needs of the SAM records and the references, made once per run: the records as Pileup.add_csr takes them
        (the alignments the host path counts its frequencies of aligned bases from), the aligned pairs of every record, and the reference /
        true base codes of every table row (npr_encode_bases' codes; rows in the order of refNames)."""
        from .utils import stageRecordsForPileup
        for aR in records:
            assert all(op in (0, 1, 2) for op, _ in aR.cigar), "callsOnDevice: %s has cigar operations other than M / I / D" % aR.qname
        # (a record is global, asserted in run(): every M column lies on the reference)
        staged = stageRecordsForPileup(sam, records, refSequences, refNames)
        trueCodes = staged["refCodes"].copy()
        for (name, i), base in snpSet.items():
            trueCodes[staged["refRows"][refIndex[name]] + i] = staged["baseCode"][ord(base)]
        staged["trueCodes"] = trueCodes
        return staged

    def _callSetsOnDevice(self, batch, staged, sampled, refLengths, hmmErrorMatrix, totalHeldOut):
        """The four call sets of one sample, in the order of the element tags, counted on the device: the two error models over the posterior
        expectations of the sampled reads, then over a pileup of the sampled records."""
        models = (FLAT_ERROR_MATRIX, hmmErrorMatrix)
        counted = batch.snp_calls(refLengths, staged["refCodes"], staged["trueCodes"], NULL_MATRIX, models, use=sampled)
        pileup = batch.ctx.pileup(refLengths)
        try:
            pileup.add_csr(staged["read"], staged["readOff"], None, staged["ops"], staged["opsOff"], staged["refIndex"], staged["start"], use=sampled)
            counted += pileup.snp_calls(staged["refCodes"], staged["trueCodes"], NULL_MATRIX, models)
        finally:
            pileup.close()
        return [SnpCalls.fromHistograms(totalHeldOut, truePos, falsePos, notCalled) for truePos, falsePos, notCalled, _ in counted]

    @staticmethod
    def _callSetsOnHost(batch, sampled, refLengths, refRows, refNames, refSequences, snpSet, hmmErrorMatrix, frequencies, seenF, totalHeldOut):
        """The four call sets of one sample from tables on the host: the posterior expectations fetched from the device, and the frequencies of
        aligned bases."""
        allE, allSeen = batch.base_expectations(refLengths, use=sampled)
        expectations = [allE[refRows[k]:refRows[k + 1]] for k in range(len(refNames))]
        seenE = [allSeen[refRows[k]:refRows[k + 1]] for k in range(len(refNames))]
        callSets = [SnpCalls(totalHeldOut) for _ in range(4)]
        configs = ((FLAT_ERROR_MATRIX, expectations, seenE), (hmmErrorMatrix, expectations, seenE),
                   (FLAT_ERROR_MATRIX, frequencies, seenF), (hmmErrorMatrix, frequencies, seenF))
        for k, refSeqName in enumerate(refNames):
            # every position of the sequence at once: candidate posteriors, then one call per non-reference base
            refCodes = _BASE_CODE[np.frombuffer(refSequences[refSeqName].encode(), dtype=np.uint8)]
            trueCodes = refCodes.copy()
            for (name, i), base in snpSet.items():
                if name == refSeqName:
                    trueCodes[i] = _BASE_CODE[ord(base)]
            for (errorM, table, seen), snpCalls in zip(configs, callSets):
                snpCalls.notCalled += int((~seen[k]).sum())
                total = table[k].sum(axis=1)
                where = np.flatnonzero(seen[k] & (total > 0.0) & (refCodes >= 0))
                if not len(where):
                    continue
                post = basePosteriors(table[k][where] / total[where, None], refCodes[where], NULL_MATRIX, errorM)
                for c in range(4):
                    called = refCodes[where] != c
                    isTrue = (trueCodes[where] != refCodes[where]) & (trueCodes[where] == c)
                    snpCalls.addCalls(post[called, c], where[called], isTrue[called])
        return callSets

    def _callsOfOneModel(self, node, hmmType, batch, records, refSequences, readSequences, refNames, alignedBases, snpSet, hmmErrorMatrix,
                         totalReferenceLength, rng, staged=None):
        """All coverages and replicates for one hmm type, on the posteriors of one batched GPU pass.  staged: callsOnDevice (_stageForDevice)."""
        batch.run()
        batch.finish()
        status = batch.results()["status"]
        for aR, st in zip(records, status):
            if st != 0:
                raise RuntimeError("Posterior computation failed for %s: status %d" % (aR.qname, st))
        refLengths = [len(refSequences[n]) for n in refNames]
        refRows = np.concatenate([[0], np.cumsum(refLengths)])
        for coverage in self.coverages:
            for replicate in range(3 if coverage < 1000000 else 1):
                order = list(range(len(records)))
                rng.shuffle(order)  # :91
                if staged is None:
                    frequencies = [np.zeros((len(refSequences[n]), 4)) for n in refNames]
                    seenF = [np.zeros(len(refSequences[n]), dtype=bool) for n in refNames]
                totalSampledReads = totalAlignedPairs = totalReadLength = 0
                sampled = np.zeros(len(records), dtype=np.uint8)
                for i in order:
                    if totalReadLength / totalReferenceLength >= coverage:  # :94
                        break
                    aR = records[i]
                    totalReadLength += len(readSequences[aR.qname])
                    totalSampledReads += 1
                    sampled[i] = 1
                    if staged is not None:
                        totalAlignedPairs += staged["alignedPairs"][i]
                        continue
                    k, pos, code = alignedBases[i]
                    totalAlignedPairs += len(pos)
                    seenF[k][pos] = True
                    ok = code >= 0
                    np.add.at(frequencies[k], (pos[ok], code[ok]), 1.0)
                totalHeldOut = len(snpSet)
                totalNotHeldOut = totalReferenceLength - totalHeldOut
                if staged is not None:
                    callSets = self._callSetsOnDevice(batch, staged, sampled, refLengths, hmmErrorMatrix, totalHeldOut)
                else:
                    callSets = self._callSetsOnHost(batch, sampled, refLengths, refRows, refNames, refSequences, snpSet, hmmErrorMatrix,
                                                    frequencies, seenF, totalHeldOut)
                tags = ("marginAlignMaxExpectedSnpCalls", "marginAlignMaxLikelihoodSnpCalls", "maxFrequencySnpCalls",
                        "maximumLikelihoodSnpCalls")
                for snpCalls, tagName in zip(callSets, tags):
                    recall = snpCalls.getRecallByProbability()
                    precision = snpCalls.getPrecisionByProbability()
                    fScore, pIndex = max((2 * recall[i] * precision[i] / (recall[i] + precision[i])
                                          if recall[i] + precision[i] > 0 else 0.0, i) for i in range(len(recall)))
                    ET.SubElement(node, tagName + "_" + hmmType, {
                        "coverage": str(coverage), "actualCoverage": str(float(totalAlignedPairs) / totalReferenceLength),
                        "totalAlignedPairs": str(totalAlignedPairs), "totalReferenceLength": str(totalReferenceLength),
                        "replicate": str(replicate), "totalReads": str(len(records)),
                        "avgSampledReadLength": str(float(totalReadLength) / max(totalSampledReads, 1)),
                        "totalSampledReads": str(totalSampledReads), "totalHeldOut": str(totalHeldOut),
                        "totalNonHeldOut": str(totalNotHeldOut), "recall": str(recall[pIndex]),
                        "precision": str(precision[pIndex]), "fScore": str(fScore),
                        "optimumProbThreshold": str(float(pIndex) / 100.0), "totalNoCalls": str(snpCalls.notCalled),
                        "recallByProbability": " ".join(map(str, recall)),
                        "precisionByProbability": " ".join(map(str, precision))})
