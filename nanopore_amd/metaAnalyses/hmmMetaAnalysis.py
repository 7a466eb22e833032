"""HmmMetaAnalysis: the trained models of all experiments of a read type, averaged.

Schema of nanopore/metaAnalyses/hmmMetaAnalysis.py.  Per read type every experiment's <experiment>/hmm.txt.xml (em.writeXML)
is collated into

  hmm_<readType>.dot                                     the five states; one edge per transition that some experiment has with
                                                         avg above 0, labelled "%.3f,%.3f" of the mean and the numpy.std of those
                                                         experiments' avgs
  matchEmissionsNormalisedByReference_<readType>.tsv     mean match emission of (x, y), divided by the sum of the row x
  matchEmissionsUnnormalised_<readType>.tsv              mean over the experiments of the match state's avg of (x, y)
  matchEmissionsUnnormalisedStdErrors_<readType>.tsv     mean over the experiments of the match state's std of (x, y)

each table with the header A C G T and one row per reference base x: `x`, then the four values.

Deliberate differences from the reference: it writes `np.average(substitutionEmissions[(b, x)][0])`, which is the mean of the
FIRST experiment's (avg, std) pair (and `[1]`, the second experiment's, for the third table: an index error with one
experiment); what was evidently meant is implemented: the mean of the avgs over all experiments for the first two tables and
the mean of the stds for the third.  A read type none of whose experiments has an hmm.txt.xml writes no files (the reference
divides by an empty mean there).  Experiments are read in the order the pipeline lists them and edges are written sorted by
(from, to).  The insert / delete emission sums the reference gathers and never writes are not gathered, and the three Rscript
plots (substitution_plot.R) are outside this project's scope and are not made.
"""
import os
import xml.etree.ElementTree as ET

import numpy as np

from ..graphviz import writeHmmGraph
from .abstractMetaAnalysis import AbstractMetaAnalysis

BASES = "ACGT"


class HmmMetaAnalysis(AbstractMetaAnalysis):
    """Averages the trained HMMs of the experiments of each read type"""

    def run(self):
        for readType in sorted(self.readTypes):
            transitions = {}                                      # (from, to) -> [avg of every experiment where it is above 0]
            avgs = {(x, y): [] for x in BASES for y in BASES}     # match state: (x, y) -> [avg of every experiment]
            stds = {(x, y): [] for x in BASES for y in BASES}
            models = 0
            for readFastqFile, experimentReadType, referenceFastaFile, mapper, analyses, resultsDir in self.experiments:
                hmmFile = os.path.join(resultsDir, "hmm.txt.xml")
                if experimentReadType != readType or not os.path.exists(hmmFile):
                    continue
                models += 1
                hmmsNode = ET.parse(hmmFile).getroot()
                for t in hmmsNode.findall("transition"):
                    if float(t.attrib["avg"]) > 0.0:
                        transitions.setdefault((t.attrib["from"], t.attrib["to"]), []).append(float(t.attrib["avg"]))
                for e in hmmsNode.findall("emission"):
                    if e.attrib["state"] == "0":
                        avgs[e.attrib["x"], e.attrib["y"]].append(float(e.attrib["avg"]))
                        stds[e.attrib["x"], e.attrib["y"]].append(float(e.attrib["std"]))
            if models == 0:
                continue
            writeHmmGraph(os.path.join(self.outputDir, "hmm_%s.dot" % readType),
                          [(a, b, "%.3f,%.3f" % (np.average(v), np.std(v))) for (a, b), v in sorted(transitions.items())])
            meanAvg = {k: float(np.average(v)) for k, v in avgs.items()}
            meanStd = {k: float(np.average(v)) for k, v in stds.items()}
            rowSum = {x: sum(meanAvg[x, y] for y in BASES) for x in BASES}
            for name, cell in (("matchEmissionsNormalisedByReference", lambda x, y: meanAvg[x, y] / rowSum[x]),
                               ("matchEmissionsUnnormalised", lambda x, y: meanAvg[x, y]),
                               ("matchEmissionsUnnormalisedStdErrors", lambda x, y: meanStd[x, y])):
                with open(os.path.join(self.outputDir, "%s_%s.tsv" % (name, readType)), "w") as outf:
                    outf.write("\t".join(BASES) + "\n")
                    for x in BASES:
                        outf.write("\t".join([x] + [str(cell(x, y)) for y in BASES]) + "\n")
