"""Base class of the unmapped-read meta-analyses: which reads did no mapper place?

Interface of nanopore/metaAnalyses/abstractUnmappedAnalysis.py.  The reference builds one `Read` object per record of every
FASTQ file (:34-35), walks every experiment's mapping.sam with pysam into a dict keyed by (qname, readFastqFile) (:37-43) and
joins the two in Python (:45-51).  Here the read database is arrays: per FASTQ file one `FastqTable` (ingest.py: the mapped
text, name spans, sequence spans, lengths) and `uint8` marks per record, set by the native join of FASTQ names with SAM
QNAMEs (`npr_names_mark`, include/nprealign.h; host code, threaded): `is_mapped`, OR-ed over every experiment of the file,
and one mark array per base mapper (first `[A-Z][a-z]*` word of `mapper.__name__`) for the mappability table.  A line
counts as the reference counts it: samIterator drops RNAME "*", then `not record.is_unmapped` (FLAG & 4 == 0).  A SAM line
that does not parse, or names a reference its header lacks, raises, as pysam's iterator does.

Differences from the reference:
  * Order.  The reference dedups reads through a Python set of (name, file, type, seq) and so iterates them in arbitrary
    order; here the order is defined: the distinct (readFastqFile, readType) pairs sorted, records in file order.  The same
    set means a record that repeats name AND sequence inside one file is one read there and one read per record here;
    records that share only the name share their marks in both.
  * Names.  A read's name is the first word of its header, which is what a mapper writes as QNAME; the reference keeps the
    whole header line and so never finds a read whose header carries a description among the QNAMEs.
  * Alignment lines whose QNAME is in no FASTQ file are counted (`strangers`), not stored.
  * `reads` is a lazy view for callers written against the reference: objects with its attributes, made on demand in the
    defined order (it scans the SAM files once more to recover the (mapper, reference) pairs).  The three analyses built on
    this class work on the arrays and never touch it.
"""
import os
import re

import numpy as np

from .. import realign
from ..ingest import FastqTable, SamText
from .abstractMetaAnalysis import AbstractMetaAnalysis


def baseMapperOf(mapper):
    return re.findall("[A-Z][a-z]*", mapper.__name__)[0]


class Read(object):
    """One read as the reference's Read presents it (abstractUnmappedAnalysis.py:8-27)."""

    def __init__(self, name, seq, readType, readFastqFile, mapRefPairs):
        self.name, self.seq, self.readType, self.readFastqFile, self.mapRefPairs = name, seq, readType, readFastqFile, mapRefPairs
        self.is_mapped = mapRefPairs is not None
        self.mappers, self.references = (set(mapRefPairs[0]), set(mapRefPairs[1])) if self.is_mapped else (None, None)

    def get_map_ref_pair(self):
        if self.mapRefPairs is not None:
            for pair in zip(self.mapRefPairs[0], self.mapRefPairs[1]):
                yield pair


class ReadFile(object):
    """The reads of one (readFastqFile, readType): `table` (FastqTable), `is_mapped` (uint8 per record) and `mapped_by`
    ({base mapper: uint8 per record}).  Entries of one file under several read types share the table and the marks, as the
    reference's (qname, readFastqFile) key shares them."""

    def __init__(self, readFastqFile, readType, table, is_mapped, mapped_by):
        self.readFastqFile, self.readType, self.table, self.is_mapped, self.mapped_by = readFastqFile, readType, table, is_mapped, mapped_by

    def names(self):
        return [self.table.name(i) for i in range(len(self.table))]


class AbstractUnmappedMetaAnalysis(AbstractMetaAnalysis):
    """Builds a database of reads and the information gathered about them during analysis"""

    def __init__(self, outputDir, experiments):
        AbstractMetaAnalysis.__init__(self, outputDir, experiments)
        self.strangers = 0  # mapped alignment lines whose QNAME is in no FASTQ file of their experiment
        byPath = {}
        for readFastqFile, readType in sorted(self.readFastqFiles):
            if readFastqFile not in byPath:
                table = FastqTable(readFastqFile)
                byPath[readFastqFile] = (table, np.zeros(len(table), dtype=np.uint8), {})
        for experiment in self.experiments:
            table, is_mapped, mapped_by = byPath[experiment[0]]
            mark, strangers = self._experimentMarks(table, experiment)
            self.strangers += strangers
            is_mapped |= mark
            base = baseMapperOf(experiment[3])
            if base in mapped_by:
                mapped_by[base] |= mark
            else:
                mapped_by[base] = mark
        self.readFiles = [ReadFile(f, t, *byPath[f]) for f, t in sorted(self.readFastqFiles)]

    def _experimentMarks(self, table, experiment):
        """(uint8 per record of the experiment's FASTQ file: mapped by its mapping.sam; mapped lines of reads the file does not have)"""
        sam = SamText(os.path.join(experiment[5], "mapping.sam"))
        mark = np.zeros(len(table), dtype=np.uint8)
        try:
            strangers = realign.names_mark(table.text, table.name_span, sam.text, sam.span, sam.parse(), mark)
        except realign.NprError:
            raise ValueError("%s: an alignment line that does not parse, or an RNAME that is not among the header's @SQ lines" % sam.path)
        return mark, strangers

    @property
    def reads(self):
        """The reference's `self.reads`, lazily: one Read per record, in the defined order."""
        for rf in self.readFiles:
            pairs, marks = [], []
            for experiment in self.experiments:
                if experiment[0] != rf.readFastqFile:
                    continue
                pair, mark = (experiment[3].__name__, experiment[2]), self._experimentMarks(rf.table, experiment)[0]
                if pair in pairs:
                    marks[pairs.index(pair)] |= mark
                else:
                    pairs.append(pair)
                    marks.append(mark)
            for i in range(len(rf.table)):
                mine = [p for p, m in zip(pairs, marks) if m[i]]
                yield Read(rf.table.name(i), rf.table.sequence(i), rf.readType, rf.readFastqFile, tuple(zip(*mine)) if mine else None)
