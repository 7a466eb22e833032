"""Base class of the meta-analyses (interface of nanopore/metaAnalyses/abstractMetaAnalysis.py:7-32): the experiments as
the pipeline hands them over, (readFastqFile, readType, referenceFastaFile, mapper, analyses, resultsDir) each, and the
sets the subclasses group them by."""
import re

from ..bioio import Target


class AbstractMetaAnalysis(Target):
    def __init__(self, outputDir, experiments):
        Target.__init__(self)
        self.experiments = experiments
        self.outputDir = outputDir
        # ((readFastqFile, readType), referenceFastaFile, mapper) -> (analyses, resultsDir)
        self.experimentHash = {}
        self.mappers = set()
        self.readFastqFiles = set()       # (readFastqFile, readType)
        self.referenceFastaFiles = set()
        self.readTypes = set()
        self.baseMappers = set()          # Lastz, Last, Bwa, Blasr: the first word of the mapper's class name
        for readFastqFile, readType, referenceFastaFile, mapper, analyses, resultsDir in self.experiments:
            self.experimentHash[((readFastqFile, readType), referenceFastaFile, mapper)] = (analyses, resultsDir)
            self.mappers.add(mapper)
            self.readFastqFiles.add((readFastqFile, readType))
            self.referenceFastaFiles.add(referenceFastaFile)
            self.readTypes.add(readType)
            self.baseMappers.add(re.findall("[A-Z][a-z]*", mapper.__name__)[0])
