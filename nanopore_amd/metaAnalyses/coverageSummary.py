"""CoverageSummary: the GlobalCoverage results of every experiment side by side, as CSV tables.

Schema of nanopore/metaAnalyses/coverageSummary.py.  `build_db` collects, per experiment that has one, the root of
<experiment>/analysis_GlobalCoverage/coverage_bestPerRead.xml (written by analyses/coverage.py).  Three groupings each write,
per group, <name>.csv and <name>_distribution.csv through `write_file_analyze`:

  by_mapper_readtype_reference   <base mapper>_<read type>_<reference file>
  by_mapper_readfile             <base mapper>_<read file>
  by_reference                   <reference file>                             (row names carry the read type)

<name>.csv has the reference's fourteen columns; the nine numbers are the root's attributes copied as the strings they are
(avgreadCoverage, avgreferenceCoverage, avgidentity, avgmismatchesPerReadBase, avgdeletionsPerReadBase,
avginsertionsPerReadBase, numberOfMappedReads, numberOfUnmappedReads, numberOfReads).  <name>_distribution.csv has per entry its
row name and the values of `distributionidentity`.  Rows are sorted by (mapper, read type, read file); a row is named after its
mapper (by_reference: <mapper>_<read type>), and where several rows of a table share that name the first keeps it and the
later ones get `.2`, `.3`, ... (`resolve_duplicate_rownames`).

Deliberate differences from the reference: a group without entries writes nothing (the reference takes entries[0] there and
raises an index error); groups are visited in sorted order, not in the order of a set; the two Rscript plots per table
(coverageSummaryPlots.R, coveragePlots.R) are outside this project's scope and are not made.
"""
import os
import re
import xml.etree.ElementTree as ET

from .abstractMetaAnalysis import AbstractMetaAnalysis

COLUMNS = ("Name", "Mapper", "ReadType", "ReadFile", "ReferenceFile", "AvgReadCoverage", "AvgReferenceCoverage", "AvgIdentity",
           "AvgMismatchesPerReadBase", "AvgDeletionsPerReadBase", "AvgInsertionsPerReadBase", "NumberOfMappedReads",
           "NumberOfUnmappedReads", "NumberOfReads")
# the root attribute behind each of the nine number columns, in column order
ATTRIBUTES = ("avgreadCoverage", "avgreferenceCoverage", "avgidentity", "avgmismatchesPerReadBase", "avgdeletionsPerReadBase",
              "avginsertionsPerReadBase", "numberOfMappedReads", "numberOfUnmappedReads", "numberOfReads")


class Entry(object):
    """One experiment's coverage result: file basenames, the mapper's class name and base mapper, the XML root."""

    def __init__(self, readType, readFastqFile, referenceFastaFile, mapper, XML):
        self.readType = readType
        self.readFastqFile = os.path.basename(readFastqFile)
        self.referenceFastaFile = os.path.basename(referenceFastaFile)
        self.mapper = mapper.__name__
        self.base_mapper = re.findall("[A-Z][a-z]*", mapper.__name__)[0]
        self.XML = XML


class CoverageSummary(AbstractMetaAnalysis):
    """Calculates meta-coverage across all the samples: per mapper, per read type + mapper, per reference, and combined"""

    def build_db(self):
        db = []
        for readFastqFile, readType, referenceFastaFile, mapper, analyses, resultsDir in self.experiments:
            path = os.path.join(resultsDir, "analysis_GlobalCoverage", "coverage_bestPerRead.xml")
            if os.path.exists(path):
                db.append(Entry(readType, readFastqFile, referenceFastaFile, mapper, ET.parse(path).getroot()))
        return db

    def _grouped(self, key):
        groups = {}
        for entry in self.db:
            groups.setdefault(key(entry), []).append(entry)
        return sorted(groups.items())

    def by_mapper_readtype_reference(self):
        for key, entries in self._grouped(lambda e: (e.base_mapper, e.readType, e.referenceFastaFile)):
            self.write_file_analyze(entries, "_".join(key))

    def by_mapper_readfile(self):
        for key, entries in self._grouped(lambda e: (e.base_mapper, e.readFastqFile)):
            self.write_file_analyze(entries, "_".join(key))

    def by_reference(self):
        for referenceFastaFile, entries in self._grouped(lambda e: e.referenceFastaFile):
            self.write_file_analyze(entries, referenceFastaFile, multiple_read_types=True)

    def write_file_analyze(self, entries, name, multiple_read_types=False):
        if not entries:
            return
        entries = sorted(entries, key=lambda e: (e.mapper, e.readType, e.readFastqFile))
        names = self.resolve_duplicate_rownames(entries, multiple_read_types)
        with open(os.path.join(self.outputDir, name + ".csv"), "w") as outf:
            outf.write(",".join(COLUMNS) + "\n")
            for entry, n in zip(entries, names):
                outf.write(",".join([n, entry.mapper, entry.readType, entry.readFastqFile, entry.referenceFastaFile]
                                    + [entry.XML.attrib[a] for a in ATTRIBUTES]) + "\n")
        with open(os.path.join(self.outputDir, name + "_distribution.csv"), "w") as outf:
            for entry, n in zip(entries, names):
                outf.write(",".join([n] + entry.XML.attrib["distributionidentity"].split()) + "\n")

    def resolve_duplicate_rownames(self, entries, multiple_read_types=False):
        """Row names of entries sorted as write_file_analyze sorts them: equal names stand next to each other."""
        names, seen = [], {}
        for entry in entries:
            n = entry.mapper + "_" + entry.readType if multiple_read_types else entry.mapper
            seen[n] = seen.get(n, 0) + 1
            names.append(n if seen[n] == 1 else "%s.%d" % (n, seen[n]))
        return names

    def run(self):
        self.db = self.build_db()
        self.by_mapper_readtype_reference()
        self.by_mapper_readfile()
        self.by_reference()
