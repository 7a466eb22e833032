"""MarginAlignMetaAnalysis: the MarginAlignSnpCaller results of every experiment as tables.

Schema of nanopore/metaAnalyses/marginAlignMetaAnalysis.py:9-131.  Every element of
<experiment>/analysis_MarginAlignSnpCaller/marginaliseConsensus.xml (written by analyses/marginAlignSnpCaller.py) is one sample: its tag
names the calling algorithm and the hmm type, its attributes the coverage asked for, the replicate and the results.  Samples are
grouped by (read type, mapper, tag, held-out proportion, reference file) and, inside a group, by coverage:

  * coverage 10 is dropped; a coverage above 1000 ("all reads") becomes `ALL`;
  * the held-out proportion totalHeldOut / (totalHeldOut + totalNonHeldOut) is snapped to 0.01 (below 0.04), 0.05 (below 0.09),
    0.1 (below 0.18) or 0.2; a sample without held-out positions is skipped.

Files:

  marginAlignAll.txt        per group and coverage: min / median / max over the replicates of fScore, recall, precision, the
                            fraction of positions not called, and the actual coverage
  marginAlignSquares.txt    per group one row: min / average / max of recall, then precision, then fScore, per coverage
  <readType>_<Mapper>.tsv   per (algorithm, proportion, coverage) two rows, `FPR` with the replicates' average
                            precisionByProbability and `TPR` with their average recallByProbability, both cut where the recall's
                            trailing zeros begin (the row labels are the reference's)

Coverages are listed numbers first, ascending, then `ALL`.

Deliberate differences from the reference: an experiment without the XML is logged and skipped (the reference does the same by
catching every exception of the parse); a coverage counts only once a sample of it has been kept; a group that lacks a coverage
other groups have writes no marginAlignAll.txt row for it, `NA` in its marginAlignSquares.txt columns and no .tsv rows (the reference
raises KeyError); the Rscript plots (ROC_marginAlign.R) are outside this project's scope and are not made.
"""
import os
import xml.etree.ElementTree as ET
from itertools import product

import numpy as np

from .abstractMetaAnalysis import AbstractMetaAnalysis

ALL_COLUMNS = ["readType", "mapper", "caller", "%heldOut", "coverage", "fScoreMin", "fScoreMedian", "fScoreMax", "recallMin", "recallMedian",
               "recallMax", "precisionMin", "precisionMedian", "precisionMax", "%notCalledMin", "%notCalledMedian", "%notCalledMax",
               "actualCoverageMin", "actualCoverageMedian", "actualCoverageMax"]


def snappedProportion(proportionHeldOut):
    return 0.01 if proportionHeldOut < 0.04 else 0.05 if proportionHeldOut < 0.09 else 0.1 if proportionHeldOut < 0.18 else 0.2


def recall(c):
    return float(c.attrib["recall"])


def precision(c):
    return float(c.attrib["precision"])


def fScore(c):
    p, r = precision(c), recall(c)
    return 2 * p * r / (p + r) if p + r > 0 else 0


def notCalled(c):
    return float(c.attrib["totalNoCalls"]) / (float(c.attrib["totalHeldOut"]) + float(c.attrib["totalNonHeldOut"]))


def actualCoverage(c):
    return float(c.attrib["actualCoverage"])


class MarginAlignMetaAnalysis(AbstractMetaAnalysis):
    def collect(self):
        """-> ({(readType, mapper name, tag, proportion, referenceFastaFile): {coverage: [elements]}}, coverages in column order)."""
        groups, coverages = {}, set()
        for readFastqFile, readType, referenceFastaFile, mapper, analyses, resultsDir in self.experiments:
            path = os.path.join(resultsDir, "analysis_MarginAlignSnpCaller", "marginaliseConsensus.xml")
            if not os.path.exists(path):
                self.logToMaster("No MarginAlignSnpCaller result: %s" % path)
                continue
            for c in ET.parse(path).getroot():
                coverage = int(c.attrib["coverage"])
                if coverage == 10:
                    continue
                if coverage > 1000:
                    coverage = "ALL"
                heldOut, nonHeldOut = float(c.attrib["totalHeldOut"]), float(c.attrib["totalNonHeldOut"])
                if heldOut == 0:
                    continue
                key = (readType, mapper.__name__, c.tag, snappedProportion(heldOut / (heldOut + nonHeldOut)), referenceFastaFile)
                groups.setdefault(key, {}).setdefault(coverage, []).append(c)
                coverages.add(coverage)
        return groups, sorted(coverages, key=lambda v: (isinstance(v, str), v))

    def run(self):
        groups, coverages = self.collect()

        def three(values, middle):
            return "\t".join(str(v) for v in (min(values), float(middle(values)), max(values)))

        curves = {}
        with open(os.path.join(self.outputDir, "marginAlignAll.txt"), "w") as allFile, \
                open(os.path.join(self.outputDir, "marginAlignSquares.txt"), "w") as squares:
            allFile.write("\t".join(ALL_COLUMNS) + "\n")
            squares.write("\t".join(["readType", "mapper", "caller", "%heldOut"] +
                                    ["%s_%s_coverage_%s" % (stat, what, coverage) for what in ("recall", "precision", "fscore")
                                     for coverage in coverages for stat in ("min", "avg", "max")]) + "\n")
            for key in sorted(groups):
                readType, mapper, algorithm, proportion, referenceFastaFile = key
                samples = groups[key]
                head = [readType, mapper, algorithm, str(proportion)]
                for coverage in coverages:
                    if coverage in samples:
                        allFile.write("\t".join(head + [str(coverage)] + [three([f(c) for c in samples[coverage]], np.median)
                                                                         for f in (fScore, recall, precision, notCalled, actualCoverage)]) + "\n")
                squares.write("\t".join(head + [three([f(c) for c in samples[coverage]], np.average) if coverage in samples else "NA\tNA\tNA"
                                                for f in (recall, precision, fScore) for coverage in coverages]) + "\n")
                for coverage in samples:
                    # the replicates' curves averaged threshold by threshold, cut where nothing is recalled any more
                    avgRecall = np.mean([[float(v) for v in c.attrib["recallByProbability"].split()] for c in samples[coverage]], axis=0).tolist()
                    avgPrecision = np.mean([[float(v) for v in c.attrib["precisionByProbability"].split()] for c in samples[coverage]], axis=0).tolist()
                    while avgRecall and avgRecall[-1] == 0.0:
                        avgRecall.pop()
                        avgPrecision.pop()
                    curves[(readType, mapper, algorithm, proportion, coverage)] = (avgPrecision, avgRecall)
        algorithms = sorted(set(key[2] for key in groups))
        proportions = sorted(set(key[3] for key in groups))
        for readType, mapper in product(sorted(self.readTypes), sorted(m.__name__ for m in self.mappers)):
            with open(os.path.join(self.outputDir, "%s_%s.tsv" % (readType, mapper)), "w") as out:
                for algorithm, proportion, coverage in product(algorithms, proportions, coverages):
                    if (readType, mapper, algorithm, proportion, coverage) not in curves:
                        continue
                    avgPrecision, avgRecall = curves[(readType, mapper, algorithm, proportion, coverage)]
                    for label, curve in (("FPR", avgPrecision), ("TPR", avgRecall)):
                        out.write("\t".join([label, algorithm, str(proportion), str(coverage)] + [str(v) for v in curve]) + "\n")
