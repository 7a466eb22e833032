"""BamFile: alignments that already sit in a BAM file -- any current mapper piped through `samtools sort`, or a file this build wrote --
taken as a base mapper's output.  run() converts <bamDir>/<readType>/<fastq stem>.<reference stem>.bam into the experiment's SAM file on
the device (Context.bam_to_sam: include/nprealign.h, npr_bam_sam; no samtools, no pysam); the `Chain` / `Realign` / `RealignEm` /
`RealignTrainedModel` variants then do what the other mappers' variants do with their SAM.  bamDir is a class attribute: pipeline.main sets
it from --bamDir (default workingDir/alignmentBamFiles).  Not in the default mapper list.
"""
import os

from .abstractMapper import AbstractMapper
from .variants import _variant


class BamFile(AbstractMapper):
    bamDir = None

    def bamFile(self):
        stem = lambda path: os.path.splitext(os.path.basename(path))[0]
        return os.path.join(self.bamDir or "alignmentBamFiles", self.readType, "%s.%s.bam" % (stem(self.readFastqFile), stem(self.referenceFastaFile)))

    def run(self):
        from ..analyses.utils import bamToSamFile
        path = self.bamFile()
        if not os.path.isfile(path):
            raise FileNotFoundError("BamFile: no alignments for %s against %s: %s does not exist" % (self.readFastqFile, self.referenceFastaFile, path))
        bamToSamFile(path, self.outputSamFile)


_g = globals()
for _suffix, _kw in (("Chain", {}), ("Realign", {}), ("RealignEm", {"doEm": True}), ("RealignTrainedModel", {"useTrainedModel": True})):
    _cls = _variant(BamFile, _suffix, **_kw)
    _g[_cls.__name__] = _cls
del _g, _suffix, _kw, _cls
