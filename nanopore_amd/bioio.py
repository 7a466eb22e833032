"""Small stand-ins for the sonLib.bioio helpers the realign path uses (sonLib is an empty submodule in the
reference snapshot): FASTA/FASTQ readers and writer, the exonerate-cigar `PairwiseAlignment` type with its
reader/writer, `nameValue` and a temp-dir `Target` shim.  SURVEY.md Appendix A/B pin the behaviour.

Cigar text grammar (nanopore/analyses/utils.py:173-177):
    cigar: <query> <qstart> <qend> <+|-> <target> <tstart> <tend> <+|-> <score> (M|I|D <len>)*
Operation types carry the SAM numbering (M 0, I 1, D 2): realignSamFile3TargetFn copies `op.type` straight
into `aR.cigar` (utils.py:602).
"""
import os
import shutil
import tempfile


def fastaRead(fileHandleOrFile):
    """Yields (name, sequence); the name is the full header line without '>'."""
    fh = open(fileHandleOrFile) if isinstance(fileHandleOrFile, str) else fileHandleOrFile
    try:
        name, chunks = None, []
        for line in fh:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if name is not None:
                    yield name, "".join(chunks)
                name, chunks = line[1:], []
            elif line and name is not None:
                chunks.append(line.strip())
        if name is not None:
            yield name, "".join(chunks)
    finally:
        if isinstance(fileHandleOrFile, str):
            fh.close()


def fastaWrite(fileHandleOrFile, name, seq, mode="w"):
    fh = open(fileHandleOrFile, mode) if isinstance(fileHandleOrFile, str) else fileHandleOrFile
    try:
        fh.write(">%s\n" % name)
        for i in range(0, len(seq), 100):
            fh.write(seq[i:i + 100] + "\n")
    finally:
        if isinstance(fileHandleOrFile, str):
            fh.close()


def _runs(mask):
    """(starts, sizes) of the runs of True in a boolean numpy array, as uint32."""
    import numpy as np
    edge = np.diff(np.concatenate(([0], mask.astype(np.int8), [0])))
    starts, ends = np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]
    return starts.astype("<u4"), (ends - starts).astype("<u4")


def faToTwoBit(fastaFile, twoBitFile):
    """The UCSC .2bit file of a FASTA file (what the reference's track hub gets from /cluster/bin/x86_64/faToTwoBit,
    nanopore/metaAnalyses/customTrackAssemblyHub.py:83), in numpy: the header (signature 0x1A412743, version 0, sequence count, 0), the
    index (name size, name -- the first word of the header line --, offset of the record), and per sequence its size, the blocks of N / n
    (count, starts, sizes), the mask blocks of lower-case runs (the same), a reserved 0 and the bases four to a byte, first base in the
    two highest bits, T = 0, C = 1, A = 2, G = 3, N and anything else packed as T, the last byte filled with T.  Little endian."""
    import numpy as np
    records = []
    for name, seq in fastaRead(fastaFile):
        name = (name.split() or [""])[0].encode()
        if not 0 < len(name) < 256:
            raise ValueError("faToTwoBit: a sequence name of %d bytes" % len(name))
        s = np.frombuffer(seq.encode(), dtype=np.uint8)
        upper = s & 0xdf
        n_starts, n_sizes = _runs(upper == ord("N"))
        m_starts, m_sizes = _runs((s >= ord("a")) & (s <= ord("z")))
        code = np.zeros(256, dtype=np.uint8)
        code[ord("C")], code[ord("A")], code[ord("G")] = 1, 2, 3
        two = np.zeros((len(s) + 3) // 4 * 4, dtype=np.uint8)
        two[:len(s)] = code[upper]
        two = two.reshape(-1, 4)
        packed = (two[:, 0] << 6 | two[:, 1] << 4 | two[:, 2] << 2 | two[:, 3]).astype(np.uint8)
        body = b"".join([np.array([len(s), len(n_starts)], dtype="<u4").tobytes(), n_starts.tobytes(), n_sizes.tobytes(),
                         np.array([len(m_starts)], dtype="<u4").tobytes(), m_starts.tobytes(), m_sizes.tobytes(),
                         np.array([0], dtype="<u4").tobytes(), packed.tobytes()])
        records.append((name, body))
    offset = 16 + sum(1 + len(name) + 4 for name, _ in records)
    out = [np.array([0x1A412743, 0, len(records), 0], dtype="<u4").tobytes()]
    for name, body in records:
        out.append(bytes([len(name)]) + name + np.array([offset], dtype="<u4").tobytes())
        offset += len(body)
    with open(twoBitFile, "wb") as fh:
        fh.write(b"".join(out + [body for _, body in records]))


def fastqRead(fileHandleOrFile):
    """Yields (name, sequence, quality string or None); four-line records."""
    fh = open(fileHandleOrFile) if isinstance(fileHandleOrFile, str) else fileHandleOrFile
    try:
        while True:
            head = fh.readline()
            if not head:
                break
            head = head.rstrip("\r\n")
            if not head:
                continue
            if not head.startswith("@"):
                raise RuntimeError("Malformed FASTQ record header: %r" % head)
            seq = fh.readline().rstrip("\r\n")
            plus = fh.readline().rstrip("\r\n")
            qual = fh.readline().rstrip("\r\n")
            if not plus.startswith("+"):
                raise RuntimeError("Malformed FASTQ record for %s" % head)
            yield head[1:], seq, (qual if qual else None)
    finally:
        if isinstance(fileHandleOrFile, str):
            fh.close()


def reverseComplement(seq):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a", "N": "N", "n": "n"}
    return "".join(comp.get(c, c) for c in reversed(seq))


def nameValue(name, value, valueType=str):
    """'--name=value', or '' when value is None (sonLib semantics; utils.py:586)."""
    if value is None:
        return ""
    if valueType is bool:
        return "--%s" % name if value else ""
    return "--%s=%s" % (name, str(value))


class AlignmentOperation(object):
    def __init__(self, opType, length, score=0.0):
        self.type = opType
        self.length = length
        self.score = score

    def __eq__(self, other):
        return self.type == other.type and self.length == other.length


class PairwiseAlignment(object):
    PAIRWISE_MATCH = 0     # 'M'
    PAIRWISE_INDEL_Y = 1   # 'I': read (query) only
    PAIRWISE_INDEL_X = 2   # 'D': reference (target) only
    PAIRWISE_PLUS = "+"
    PAIRWISE_MINUS = "-"
    _LETTER = {0: "M", 1: "I", 2: "D"}
    _CODE = {"M": 0, "I": 1, "D": 2}

    def __init__(self, contig1, start1, end1, strand1, contig2, start2, end2, strand2, score, operationList):
        # contig1 = target (reference), contig2 = query (read): SURVEY.md Appendix A naming
        self.contig1, self.start1, self.end1, self.strand1 = contig1, start1, end1, strand1
        self.contig2, self.start2, self.end2, self.strand2 = contig2, start2, end2, strand2
        self.score = score
        self.operationList = operationList


def cigarReadFromString(line):
    tok = line.split()
    if len(tok) < 10 or tok[0] != "cigar:":
        raise RuntimeError("Malformed cigar line: %r" % line)
    ops = []
    rest = tok[10:]
    if len(rest) % 2:
        raise RuntimeError("Malformed cigar operations: %r" % line)
    for letter, length in zip(rest[::2], rest[1::2]):
        if letter not in PairwiseAlignment._CODE:
            raise RuntimeError("Unknown cigar operation %r" % letter)
        ops.append(AlignmentOperation(PairwiseAlignment._CODE[letter], int(length)))
    pA = PairwiseAlignment(tok[5], int(tok[6]), int(tok[7]), tok[8] == "+", tok[1], int(tok[2]), int(tok[3]),
                           tok[4] == "+", float(tok[9]), ops)
    qspan = sum(o.length for o in ops if o.type in (0, 1))
    tspan = sum(o.length for o in ops if o.type in (0, 2))
    if qspan != abs(pA.end2 - pA.start2) or tspan != abs(pA.end1 - pA.start1):
        raise RuntimeError("Cigar operations do not span the stated coordinates: %r" % line)
    return pA


def cigarRead(fileHandleOrFile):
    fh = open(fileHandleOrFile) if isinstance(fileHandleOrFile, str) else fileHandleOrFile
    try:
        for line in fh:
            if line.startswith("cigar:"):
                yield cigarReadFromString(line)
    finally:
        if isinstance(fileHandleOrFile, str):
            fh.close()


def cigarToString(pA):
    ops = " ".join("%s %i" % (PairwiseAlignment._LETTER[o.type], o.length) for o in pA.operationList)
    return "cigar: %s %i %i %s %s %i %i %s %s %s" % (
        pA.contig2, pA.start2, pA.end2, "+" if pA.strand2 else "-", pA.contig1, pA.start1, pA.end1,
        "+" if pA.strand1 else "-", repr(float(pA.score)) if pA.score != int(pA.score) else "%i" % pA.score, ops)


def cigarWrite(fileHandle, pA, withProbs=False):
    fileHandle.write(cigarToString(pA).rstrip() + "\n")


class Target(object):
    """The slice of jobTree's Target the realign path touches (temp dirs, logging, child / follow-on
    scheduling).  jobTree is an empty submodule in the snapshot and its engine is out of scope (SURVEY.md 2
    row 11): children run immediately and in order, follow-ons right after -- the ordering semantics the
    reference relies on at nanopore/analyses/utils.py:540-609."""

    def __init__(self, tempDir=None):
        self._own = tempDir is None
        self._dir = tempDir or tempfile.mkdtemp(prefix="nanopore_amd_")
        self._followOn = None
        self.messages = []

    def getGlobalTempDir(self):
        return self._dir

    def getLocalTempDir(self):
        return self._dir

    def logToMaster(self, message):
        self.messages.append(message)

    def addChildTargetFn(self, fn, args=()):
        fn(self, *args)

    def addChildTarget(self, target):
        target.run()

    def setFollowOnTargetFn(self, fn, args=()):
        self._followOn = (fn, args)

    def runFollowOns(self):
        while self._followOn is not None:
            fn, args = self._followOn
            self._followOn = None
            fn(self, *args)

    def cleanup(self):
        if self._own and os.path.isdir(self._dir):
            shutil.rmtree(self._dir, ignore_errors=True)
