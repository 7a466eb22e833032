"""ChannelMappability: channel_mappability.tsv, reads and mapped records per nanopore channel.

Schema of nanopore/analyses/channelMappability.py.  A name counts when it starts with `channel_<n>_read_<m>` (digits); <n>
is its channel.  ReadCount is the number of FASTQ records of a channel; MappableReadCount the number of SAM records of a
channel that have a reference and lack FLAG 4 -- one per record, as the reference counts, so a read with two records counts
twice.  The file has the header `Channel ReadCount MappableReadCount` (tabs) and one row per channel 1 .. max(513, highest
channel among the reads) - 1; it is written only when both counters hold something.

Both files are read by the native scanners (ingest.FastqTable, ingest.SamText: mapped text, name spans, parsed fields); the
only Python loop is one regular-expression match per name.  A SAM line that does not parse raises, as pysam's iterator does.
The four Rscript plots of the reference (channel_plots.R) are outside this project's scope and are not made.
"""
import os
import re
from collections import Counter

from .. import ingest
from .abstractAnalysis import AbstractAnalysis

CHANNEL_NAME = re.compile(br"channel_([0-9]+)_read_[0-9]+")
HEADER = "Channel\tReadCount\tMappableReadCount\n"


def channelCounts(text, starts, ends):
    """Counter {channel: names text[starts[i]:ends[i]] of that channel}."""
    counts = Counter()
    for a, b in zip(starts.tolist(), ends.tolist()):
        m = CHANNEL_NAME.match(bytes(text[a:b]))
        if m:
            counts[int(m.group(1))] += 1
    return counts


class ChannelMappability(AbstractAnalysis):
    """Calculates nanopore channel specific mappability"""

    def run(self):
        AbstractAnalysis.run(self)
        fq = ingest.FastqTable(self.readFastqFile)
        perChannelReadCounts = channelCounts(fq.text, fq.name_span[:, 0], fq.name_span[:, 1])
        sam = ingest.SamText(self.samFile)
        fields = sam.parse()
        mapped = sam.records_with_a_reference(fields, sam.span) & ((fields[:, ingest.F_FLAG] & 4) == 0)
        mappedReadCounts = channelCounts(sam.text, sam.span[mapped, 0], fields[mapped, ingest.F_QNAME_END])
        if len(mappedReadCounts) > 0 and len(perChannelReadCounts) > 0:
            maxChannel = max(513, max(perChannelReadCounts))  # (the reference: "in case there are more than 512 in the future")
            with open(os.path.join(self.outputDir, "channel_mappability.tsv"), "w") as outf:
                outf.write(HEADER)
                for channel in range(1, maxChannel):
                    outf.write("%d\t%d\t%d\n" % (channel, perChannelReadCounts[channel], mappedReadCounts[channel]))
        self.finish()
