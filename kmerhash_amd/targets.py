"""The contig table of a reference of several sequences: where every target stands in the one text the index is built from.

The targets are laid out one after the other, separated by `spacer` bytes of 'N'.  A byte that is no base matches nothing
(kh_chain_edits in include/kmerhash_amd.h), so crossing a spacer of at least 32 bytes costs more edits than max_edits can be (31):
neither a chain link nor an end extension crosses one, and kmers.group_anchors keeps the chaining DP inside a target.  Host code: this is
a build-time step."""
import numpy as np

from ._call import torch
from ._xp import namespace_of

TARGET_NONE = 0xFFFFFFFF          # KH_TARGET_NONE: an anchor that lies in no target
MIN_SPACER = 32                   # max_edits is at most 31


class Targets:
    """Targets(names, lengths, spacer=64): target t covers the coordinates [starts[t], ends[t]) with starts[0] = 0,
    ends[t] = starts[t] + lengths[t] and starts[t + 1] = ends[t] + spacer.  Attributes: names (list of str), lengths (int64), starts and
    ends (uint32), spacer, text (the uint8 text of from_sequences / from_fasta, else None).  ValueError for spacer < 32, no target, a
    target of length 0, a repeated name or a layout that ends beyond 2^31 (a position has 31 bits)."""

    def __init__(self, names, lengths, spacer=64):
        names = [n.decode("ascii") if isinstance(n, (bytes, bytearray)) else str(n) for n in names]
        lengths = np.asarray(lengths, dtype=np.int64).ravel()
        spacer = int(spacer)
        if spacer < MIN_SPACER:
            raise ValueError("spacer must be at least %d (more bytes that match nothing than max_edits can be), got %d" % (MIN_SPACER, spacer))
        if len(names) == 0 or len(names) != lengths.size:
            raise ValueError("one name and one length per target and at least one target, got %d names and %d lengths" % (len(names), lengths.size))
        if (lengths < 1).any():
            raise ValueError("every target must hold at least one base (target %d has length %d)" % (int(np.argmax(lengths < 1)), int(lengths.min())))
        if len(set(names)) != len(names):
            raise ValueError("target names must be unique")
        if int(lengths.sum()) + spacer * (lengths.size - 1) > 2 ** 31:
            raise ValueError("the targets with their spacers must end within 2^31 (a position has 31 bits), got %d" % (int(lengths.sum()) + spacer * (lengths.size - 1)))
        ends = np.cumsum(lengths) + spacer * np.arange(lengths.size, dtype=np.int64)
        self.names, self.lengths, self.spacer, self.text = names, lengths, spacer, None
        self.starts, self.ends = (ends - lengths).astype(np.uint32), ends.astype(np.uint32)      # (ends[-1] == 2^31 fits)
        self._dev = {}

    def __len__(self):
        return len(self.names)

    @classmethod
    def from_sequences(cls, names, seqs, spacer=64):
        """the table of the given sequences (bytes or uint8 arrays) and .text: the sequences joined by `spacer` bytes of 'N'"""
        seqs = [np.frombuffer(s.encode("ascii") if isinstance(s, str) else bytes(s), dtype=np.uint8) if isinstance(s, (str, bytes, bytearray))
                else np.asarray(s, dtype=np.uint8).ravel() for s in seqs]
        T = cls(names, [s.size for s in seqs], spacer)
        text = np.full(int(T.ends[-1]), ord("N"), dtype=np.uint8)
        for s, a in zip(seqs, T.starts):
            text[int(a):int(a) + s.size] = s
        T.text = text
        return T

    @classmethod
    def from_fasta(cls, buf, spacer=64):
        """the table and .text of FASTA bytes: a record's name is its header up to the first whitespace, its sequence the lines that
        follow with the line breaks (and any other whitespace) removed.  Bytes before the first header are ignored."""
        a = np.frombuffer(bytes(buf), dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else np.asarray(buf, dtype=np.uint8).ravel()
        nl = np.flatnonzero(a == 10)
        line_start = np.concatenate([[0], nl + 1]).astype(np.int64)
        line_start = line_start[line_start < a.size]
        heads = line_start[a[line_start] == ord(">")]
        if heads.size == 0:
            raise ValueError("no FASTA record (no line starts with '>')")
        # the end of every header line: the next line break, or the end of the text; a record's body runs from there to the next header
        head_end = np.concatenate([nl, [a.size]]).astype(np.int64)[np.searchsorted(nl, heads)]
        body_end = np.concatenate([heads[1:], [a.size]]).astype(np.int64)
        fields = [bytes(a[h + 1:e]).split() for h, e in zip(heads, head_end)]
        if not all(fields):
            raise ValueError("a FASTA header without a name")
        names = [f[0].decode("ascii") for f in fields]
        # a sequence byte: inside a record's body and no whitespace
        keep = ~np.isin(a, np.frombuffer(b" \t\r\n\v\f", dtype=np.uint8))
        mark = np.zeros(a.size + 1, dtype=np.int64)      # +1 at the start of a body, -1 at its end
        np.add.at(mark, head_end, 1)
        np.add.at(mark, body_end, -1)
        keep &= np.cumsum(mark[:-1]) > 0
        kept = np.concatenate([[0], np.cumsum(keep)])
        lengths = kept[body_end] - kept[head_end]
        T = cls(names, lengths, spacer)
        text = np.full(int(T.ends[-1]), ord("N"), dtype=np.uint8)
        seq = a[keep]
        # the kept bytes stand record by record: a byte of record r moves up by r spacers
        rec = np.repeat(np.arange(lengths.size, dtype=np.int64), lengths)
        text[np.arange(seq.size, dtype=np.int64) + rec * T.spacer] = seq
        T.text = text
        return T

    def to(self, device):
        """(starts, ends) as int32 CUDA tensors holding the uint32 bits, cached per device"""
        dev = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.starts.view(np.int32)).to(dev), torch.from_numpy(self.ends.view(np.int32)).to(dev))
        return self._dev[key]

    def locate(self, pos):
        """positions -> (target, local): the target every position lies in and its offset from that target's start; target -1 (and local
        0) for a position in a spacer or beyond the last target.  numpy in (any integer dtype; uint32 bits in an int32 array are read as
        uint32), numpy int64 out; a CUDA tensor in (int32 holding uint32 bits, or int64), int64 tensors out."""
        return self.locate_on(namespace_of(pos), pos)

    def bound(self, xp, end):
        """starts (end = 0) or ends (end = 1) as an int64 column of the namespace xp"""
        return (self.starts, self.ends)[end].astype(np.int64) if xp.host else xp.widen(self.to(xp.device)[end])

    def locate_on(self, xp, pos):
        """locate() over the array namespace xp (kmerhash_amd._xp), where pos lives"""
        p = xp.widen(pos)
        starts, ends = self.bound(xp, 0), self.bound(xp, 1)
        t = xp.searchsorted(starts, p, right=True) - 1
        tc = xp.maximum(t, 0)
        ok = (t >= 0) & (p < ends[tc])
        return xp.where(ok, t, xp.full(len(t), -1)), xp.where(ok, p - starts[tc], xp.full(len(p), 0))


def inside_target(xp, targets, rs, re_):
    """the half of the printable-row rule that needs the contig table: the interval [rs, re) (uint32 bits or int64) lies inside one
    target -- its first base in a target, its end not beyond that target's end -> (inside, target per row, -1: none)"""
    tgt, _ = targets.locate_on(xp, rs)
    return (tgt >= 0) & (xp.widen(re_) <= targets.bound(xp, 1)[xp.maximum(tgt, 0)]), tgt
