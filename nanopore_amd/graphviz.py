"""The four graphviz writers the Hmm analysis and the HmmMetaAnalysis draw the model with (names and argument order of the
sonLib.bioio helpers nanopore/analyses/hmm.py:22-39 calls; sonLib is an empty submodule in the reference snapshot).  The file
is plain DOT: `graph G { ... }`, one `name [attributes];` per node, one `a -- b [attributes];` per edge.  Every attribute value
is written as a quoted string, so labels may hold blanks and commas.
"""


def _quote(value):
    return '"%s"' % str(value).replace("\\", "\\\\").replace('"', '\\"')


def _attributes(pairs):
    return ", ".join("%s=%s" % (key, _quote(value)) for key, value in pairs if value is not None and value != "")


def setupGraphFile(graphFileHandle):
    graphFileHandle.write("graph G {\n")
    graphFileHandle.write("overlap=false;\n")


def addNodeToGraph(nodeName, graphFileHandle, label, width=0.3, height=0.3, shape="circle", colour="black", fontsize=14):
    graphFileHandle.write("%s [%s];\n" % (nodeName, _attributes([("label", label), ("width", width), ("height", height), ("shape", shape),
                                                                 ("color", colour), ("fontsize", fontsize)])))


def addEdgeToGraph(parentNodeName, childNodeName, graphFileHandle, colour="black", length="10", weight="1", dir="none", label="", style=""):
    """`dir`: graphviz's forward / back / both / none; "arrow" (what the model drawings ask for) is written as forward."""
    graphFileHandle.write("%s -- %s [%s];\n" % (parentNodeName, childNodeName, _attributes([
        ("label", label), ("color", colour), ("len", length), ("weight", weight), ("dir", "forward" if dir == "arrow" else dir), ("style", style)])))


def finishGraphFile(graphFileHandle):
    graphFileHandle.write("}\n")


# the five states of the pair-HMM as the drawings name them (hmm.py:24-28)
STATE_NODES = (("n0n", "match"), ("n1n", "short delete"), ("n2n", "short insert"), ("n3n", "long insert"), ("n4n", "long delete"))


def writeHmmGraph(path, edges):
    """The model drawing both hmm plugins write: the five state nodes, then one edge per (fromState, toState, label)."""
    with open(path, "w") as fH:
        setupGraphFile(fH)
        for name, label in STATE_NODES:
            addNodeToGraph(name, fH, label)
        for fromState, toState, label in edges:
            addEdgeToGraph("n%sn" % fromState, "n%sn" % toState, fH, dir="arrow", label=label)
        finishGraphFile(fH)
