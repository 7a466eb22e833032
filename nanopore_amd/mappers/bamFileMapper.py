"""BamFile: alignments that already sit in a BAM file -- any current mapper piped through `samtools sort`, or a file this build wrote --
taken as a base mapper's output.  run() converts <bamDir>/<readType>/<fastq stem>.<reference stem>.bam into the experiment's SAM file on
the device (Context.bam_to_sam: include/nprealign.h, npr_bam_sam; no samtools, no pysam); the `Chain` / `Realign` / `RealignEm` /
`RealignTrainedModel` variants then do what the other mappers' variants do with their SAM.  bamDir is a class attribute: pipeline.main sets
it from --bamDir (default workingDir/alignmentBamFiles).  Not in the default mapper list.
CombinedBamFile: the counterpart of the reference's CombinedMapper* (combineSamFiles over several mappers' outputs): every
<bamDir>/<readType>/<fastq stem>.<reference stem>.*.bam, in the order of the file names, merged on the device one file after the other
(bam.bam_merge with sort=False: include/nprealign.h, npr_bam_streams_bam) and written as the experiment's SAM file under the first file's
header.  The same four variants; not in the default list either.
"""
import glob
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


class CombinedBamFile(BamFile):
    def bamPattern(self):
        return self.bamFile()[:-len(".bam")] + ".*.bam"

    def run(self):
        import numpy as np
        from ..analyses.utils import _context
        paths = sorted(glob.glob(glob.escape(self.bamPattern()[:-len(".*.bam")]) + ".*.bam"), key=os.path.basename)
        if not paths:
            raise FileNotFoundError("CombinedBamFile: no alignments for %s against %s: no file matches %s" % (self.readFastqFile, self.referenceFastaFile, self.bamPattern()))
        ctx, streams = _context(), []
        try:
            for path in paths:
                streams.append(ctx.bam_open(np.fromfile(path, dtype=np.uint8)))
            image, _ = ctx.bam_merge(streams, sort=False, index=False)
        finally:
            for s in streams:
                s.close()
        with ctx.bam_open(image) as merged:
            text = merged.sam_text()
        tmp = self.outputSamFile + ".tmp"
        try:
            with open(tmp, "wb") as fh:
                text.tofile(fh)
            os.replace(tmp, self.outputSamFile)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)


_g = globals()
for _base in (BamFile, CombinedBamFile):
    for _suffix, _kw in (("Chain", {}), ("Realign", {}), ("RealignEm", {"doEm": True}), ("RealignTrainedModel", {"useTrainedModel": True})):
        _cls = _variant(_base, _suffix, **_kw)
        _g[_cls.__name__] = _cls
del _g, _base, _suffix, _kw, _cls
