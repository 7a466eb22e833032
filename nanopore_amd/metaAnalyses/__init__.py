"""Meta-analyses: what the reference computes over the result directories of several experiments (nanopore/metaAnalyses/)."""
