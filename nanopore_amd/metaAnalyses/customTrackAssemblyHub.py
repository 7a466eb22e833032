"""CustomTrackAssemblyHub: a UCSC assembly hub of every experiment's alignments.

Layout and text of nanopore/metaAnalyses/customTrackAssemblyHub.py:35-131: under the meta-analysis directory one folder per reference
FASTA file (its name up to ".fa") holding the FASTA file, its .2bit, trackDb.txt and bamFiles/<experiment>.sorted.bam + .bai;
genomes.txt and groups.txt beside the folders.  The reference makes the files with samToBamFile, pysam.sort, pysam.index and the
faToTwoBit binary; here the sorted BAM and its index come from the device (analyses/utils.samToSortedBamFile, csrc/npr_bam.hip) and the
.2bit from bioio.faToTwoBit.  No external binary, no CPU fallback.

Deliberate differences.  The reference derives an experiment's folder from the experiment directory's name
(`experiment.split(".fastq")[-1].split(".fa")[0][1:]`), which names the reference only for read files ending in ".fastq"; here the folder
comes from the experiment's own reference file, the same thing for such names.  The reference appends to the three text files, so a second
run repeats every stanza; here they are written anew.  The reference swallows a failed conversion (`except: continue`); here the other
experiments are still converted and the failures are raised together afterwards, which the pipeline driver reports as a failed
meta-analysis.  The reference does its work in __init__; here it is run().  Not in the pipeline's default list (the reference has it
commented out there): `--metaAnalyses CustomTrackAssemblyHub`.  CustomTrackAssemblyHubCompressed lays out the same hub with BAM files
whose BGZF blocks are compressed on the device (csrc/npr_deflate.hip), as the reference's are: a browser fetches them over HTTP.
"""
import os
import shutil

from ..bioio import faToTwoBit, fastaRead
from .abstractMetaAnalysis import AbstractMetaAnalysis

GROUPS_TEXT = "name readType\nlabel readType\npriority 1\ndefaultIsClosed 0\n\n"


def referenceHeader(referenceFastaFile):
    return referenceFastaFile.split("/")[-1].split(".fa")[0]


def trackDbText(experiment, trackLabel):
    """One experiment's stanza of trackDb.txt (customTrackAssemblyHub.py:106-120)."""
    readType = experiment.split(".fastq")[0].split("_")[-1]
    shortLabel = experiment.strip().split("_")[-1]
    return ("track " + str(trackLabel) + "_\n" + "longLabel " + experiment + "\n" + "shortLabel " + readType + "_" + shortLabel + "\n" +
            "priority 10\n" + "visibility pack\n" + "colorByStrand 150,100,30 230,170,40\n" + "color 150,100,30\n" + "altColor 230,170,40\n" +
            "bigDataUrl bamFiles/" + experiment + ".sorted.bam\n" + "type bam\n" + "group " + readType + "\n" + "html assembly\n\n")


def genomesText(header, sequenceId, length):
    """One reference's stanza of genomes.txt (customTrackAssemblyHub.py:93-100); the position is that of the file's LAST sequence."""
    return ("genome " + header + "\n" + "trackDb " + header + "/trackDb.txt\n" + "groups groups.txt\n" + "description " + header + "\n" +
            "twoBitPath " + header + "/" + header + ".2bit\n" + "organism " + header + "\n" + "defaultPos " + sequenceId + ":1-" + str(length) + "\n" + "\n")


class CustomTrackAssemblyHub(AbstractMetaAnalysis):
    """mapping.sam of every experiment as <reference>/bamFiles/<experiment>.sorted.bam + .bai, with trackDb.txt, genomes.txt, groups.txt"""

    compress = False   # stored BGZF blocks; the subclass below compresses them

    def run(self, ctx=None):
        from ..analyses.utils import samToSortedBamFile
        failed, tracks = [], {}
        trackLabel = 1
        for readFastqFile, readType, referenceFastaFile, mapper, analyses, resultsDir in self.experiments:
            experiment = resultsDir.rstrip("/").split("/")[-1]
            hubDir = os.path.join(self.outputDir, referenceHeader(referenceFastaFile))
            bamDir = os.path.join(hubDir, "bamFiles")
            os.makedirs(bamDir, exist_ok=True)
            try:   # (the keyword only when set: a converter put in this one's place with the plain signature keeps working)
                samToSortedBamFile(os.path.join(resultsDir, "mapping.sam"), os.path.join(bamDir, experiment + ".sorted.bam"), ctx=ctx, **({"compress": True} if self.compress else {}))
            except Exception as e:  # the other experiments still get their files
                failed.append((experiment, e))
                continue
            tracks.setdefault(hubDir, []).append(trackDbText(experiment, trackLabel))
            trackLabel += 1
        genomes = []
        for referenceFastaFile in sorted(self.referenceFastaFiles):
            if not (referenceFastaFile.endswith(".fa") or referenceFastaFile.endswith(".fasta")):
                continue
            header = referenceHeader(referenceFastaFile)
            hubDir = os.path.join(self.outputDir, header)
            os.makedirs(hubDir, exist_ok=True)
            copy = os.path.join(hubDir, os.path.basename(referenceFastaFile))
            shutil.copyfile(referenceFastaFile, copy)
            faToTwoBit(copy, os.path.join(hubDir, header + ".2bit"))
            sequenceId, length = "", 0
            for name, seq in fastaRead(referenceFastaFile):
                sequenceId, length = name.split(" ")[0], len(seq)
            genomes.append(genomesText(header, sequenceId, length))
        for hubDir, stanzas in tracks.items():
            with open(os.path.join(hubDir, "trackDb.txt"), "w") as fh:
                fh.write("".join(stanzas))
        with open(os.path.join(self.outputDir, "genomes.txt"), "w") as fh:
            fh.write("".join(genomes))
        with open(os.path.join(self.outputDir, "groups.txt"), "w") as fh:
            fh.write(GROUPS_TEXT)
        if failed:
            raise RuntimeError("CustomTrackAssemblyHub: no sorted BAM for %s" % ", ".join("%s (%s: %s)" % (x, type(e).__name__, e) for x, e in failed)) from failed[0][1]


class CustomTrackAssemblyHubCompressed(CustomTrackAssemblyHub):
    """The same hub with compressed BAM files (`--metaAnalyses CustomTrackAssemblyHubCompressed`; not in the default list either)"""
    compress = True
