"""Hmm: the trained model of an experiment as a drawing and three tables.

Schema of nanopore/analyses/hmm.py (the module is hmmAnalysis.py here: nanopore_amd/hmm.py is the model class).  The input
is `hmm.txt.xml` next to the experiment's mapping.sam, which em.writeXML writes when a *RealignEm mapper trained the model
(`transition from/to/avg/std`, `emission state/x/y/avg/std`, one `hmm runningLikelihoods` per trial).  Without that file the
analysis only marks itself finished.  Otherwise it writes

  hmm.dot                  the five states, one edge per transition whose avg is above 0, labelled "avg,std" to three decimals
  matchEmissions.tsv       header A C G T; per reference base x a row `x` and the match state's avg of (x, A) .. (x, T), the
                           XML's strings as they are
  indelEmissions.tsv       the same header; the short-insert state's avgs summed by x; the short-delete state's summed by y
  runninglikelihoods.tsv   per trial one line: its running likelihoods, first iteration first

The plots the reference makes of the three tables with Rscript (substitution_plot.R, emissions_plot.R, running_likelihood.R)
are outside this project's scope and are not made; nor are the FASTA and FASTQ dictionaries loaded that the reference reads
there and never uses.
"""
import os
import xml.etree.ElementTree as ET

from ..graphviz import writeHmmGraph
from .abstractAnalysis import AbstractAnalysis

BASES = "ACGT"
MATCH_STATE, SHORT_DELETE_STATE, SHORT_INSERT_STATE = "0", "1", "2"


class Hmm(AbstractAnalysis):
    """Tables and a drawing of the experiment's trained HMM"""

    def run(self):
        AbstractAnalysis.run(self)
        hmmFile = os.path.join(os.path.split(self.samFile)[0], "hmm.txt.xml")
        if os.path.exists(hmmFile):
            hmmsNode = ET.parse(hmmFile).getroot()
            writeHmmGraph(os.path.join(self.outputDir, "hmm.dot"),
                          [(t.attrib["from"], t.attrib["to"], "%.3f,%.3f" % (float(t.attrib["avg"]), float(t.attrib["std"])))
                           for t in hmmsNode.findall("transition") if float(t.attrib["avg"]) > 0.0])
            match = {}
            inserts, deletes = dict.fromkeys(BASES, 0.0), dict.fromkeys(BASES, 0.0)
            for e in hmmsNode.findall("emission"):
                if e.attrib["state"] == MATCH_STATE:
                    match[e.attrib["x"], e.attrib["y"]] = e.attrib["avg"]
                elif e.attrib["state"] == SHORT_INSERT_STATE:
                    inserts[e.attrib["x"]] += float(e.attrib["avg"])
                elif e.attrib["state"] == SHORT_DELETE_STATE:
                    deletes[e.attrib["y"]] += float(e.attrib["avg"])
            header = "\t".join(BASES) + "\n"
            with open(os.path.join(self.outputDir, "matchEmissions.tsv"), "w") as outf:
                outf.write(header)
                for x in BASES:
                    outf.write("\t".join([x] + [match[x, y] for y in BASES]) + "\n")
            with open(os.path.join(self.outputDir, "indelEmissions.tsv"), "w") as outf:
                outf.write(header)
                for sums in (inserts, deletes):
                    outf.write("\t".join(str(sums[b]) for b in BASES) + "\n")
            with open(os.path.join(self.outputDir, "runninglikelihoods.tsv"), "w") as outf:
                for hmmNode in hmmsNode.findall("hmm"):
                    outf.write("\t".join(str(float(v)) for v in hmmNode.attrib["runningLikelihoods"].split()) + "\n")
        self.finish()
