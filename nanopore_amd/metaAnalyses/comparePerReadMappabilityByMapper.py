"""ComparePerReadMappabilityByMapper: <readType>_perReadMappability.tsv, which base mappers placed which reads.

Schema of nanopore/metaAnalyses/comparePerReadMappabilityByMapper.py:11-25: a header `Read`, `ReadFastqFile` and one column
per base mapper (first `[A-Z][a-z]*` word of the mapper's class name) sorted by name, `Combined` left out; one row per read
of the read type with the read's name, the basename of its FASTQ file and 0 / 1 per base mapper.  The columns are the mark
arrays of the read database (abstractUnmappedAnalysis.py).  Differences: rows in the defined order of the read database;
the `Rscript` Venn diagram is left out.
"""
import os

from .abstractUnmappedAnalysis import AbstractUnmappedMetaAnalysis


class ComparePerReadMappabilityByMapper(AbstractUnmappedMetaAnalysis):
    """Finds which base mappers mapped which reads"""

    def run(self):
        sortedBaseMappers = [x for x in sorted(self.baseMappers) if x != "Combined"]
        for readType in sorted(self.readTypes):
            with open(os.path.join(self.outputDir, readType + "_perReadMappability.tsv"), "w") as outf:
                outf.write("Read\tReadFastqFile\t" + "\t".join(sortedBaseMappers) + "\n")
                for rf in self.readFiles:
                    if rf.readType != readType:
                        continue
                    base = os.path.basename(rf.readFastqFile)
                    columns = [rf.mapped_by[x].tolist() if x in rf.mapped_by else [0] * len(rf.table) for x in sortedBaseMappers]
                    for i, name in enumerate(rf.names()):
                        outf.write("\t".join([name, base] + [str(c[i]) for c in columns]) + "\n")
