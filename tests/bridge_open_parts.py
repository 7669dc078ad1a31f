"""The yardstick of tests/test_gpu_bridge_open.py: tests/bridge_parts.py's chains of C-ABI batches called one by one, for a
bridge whose seats change hands (mi_bridge_create_open, mi_bridge_change_members).  The chains have their batches for EVERY
admitted rate from the start -- an MSVolume batch and both resampler batches per rate, a concealer batch per rate --, each
over all n streams with a run mask for the streams that are its own, so a new endpoint on a seat is a relabelling of the
seat plus restart(s): fresh meter, fresh resamplers, fresh concealer in the batch of ITS rate.  The pitches and the buffers'
widths come from the union of the kinds, as the bridge's do.  bridge_parts.py is used as it stands: tick(), decode(), rows(),
restart() and the state read-outs are Parts' own."""
import numpy as np

import mediastreamer2_amd as ms
from bridge_parts import LAW, PCM16, ConcealedParts, Parts, _Legs

L, A, O = ms.MI_MIX_LINKED, ms.MI_MIX_ACTIVE, ms.MI_MIX_OUTPUT


def union(legs, admit):
    """the distinct kinds of the legs and the admitted ones, in order of appearance"""
    return list(dict.fromkeys([tuple(int(v) for v in k) for k in list(legs) + list(admit)]))


class _Seats:
    """what both chains share: a seat's label -- rate, codecs, and everything _Legs / Parts derive from them per leg"""

    def relabel(self, s, kind):
        self.rates[s], self.ic[s], self.oc[s] = kind
        self.derive()

    def derive(self):
        self.leg_len = self.rates // 100
        self.in_bytes = self.leg_len * np.where(self.ic, 1, 2)
        self.out_bytes = self.leg_len * np.where(self.oc, 1, 2)
        self.lens = self._dev(self.leg_len.astype(np.int32))
        self.law_in = {c: self._dev(np.where(self.ic == c, self.leg_len, 0).astype(np.int32)) for c in LAW if (self.ic == c).any()}
        self.t.cuda.synchronize()


class OpenParts(_Seats, Parts):
    """Parts for the union: batches for every rate of `kinds`, byte rows at the union's pitches"""

    def __init__(self, ctx, mk, mm, conf, legs, admit):
        kinds = union(legs, admit)
        self.mm, self.conf, self.ns = mm, conf, conf // 100
        widest = max(k[0] for k in kinds) // 100
        _Legs.__init__(self, ctx, legs, lambda _: max(self.ns, widest) + 8)
        n, torch = self.n, self.t
        up = lambda v: -(-v // self.ALIGN) * self.ALIGN
        self.in_pitch = up(max(k[0] // 100 * (1 if k[1] else 2) for k in kinds))
        self.out_pitch = up(max(k[0] // 100 * (1 if k[2] else 2) for k in kinds))
        self.distinct = sorted(set(k[0] for k in kinds))
        self.vol = {r: mk(ms.VolumeBatch, n, r) for r in self.distinct}
        self.res_in = {r: mk(ms.ResamplerBatch, n, r, conf) for r in self.distinct if r != conf}
        self.res_out = {r: mk(ms.ResamplerBatch, n, conf, r) for r in self.distinct if r != conf}
        self.mix = mk(ms.MixerBatch, n // mm, mm, self.ns)
        self.plc = None
        self.flags = np.full(n, L | A | O, np.uint8)
        self.gain = np.ones(n, np.float32)
        self.held = np.zeros((3, n, self.out_pitch), np.uint8)  # (a row that is not written keeps what ITS staging slot held)
        self.ticks = 0
        z = lambda cols, dt=torch.int16: torch.zeros((n, cols), dtype=dt, device="cuda")
        self.back = z(self.width)
        self.wide, self.mixed = z(self.ns), z(self.ns)
        self.narrow = z(self.ns + 8)
        self.codes_out = z(self.out_pitch, torch.uint8)
        self.derive()

    def derive(self):
        super().derive()
        self.law_out = {c: self._dev(np.where(self.oc == c, self.leg_len, 0).astype(np.int32)) for c in LAW if (self.oc == c).any()}
        self.t.cuda.synchronize()

    def leave_seat(self, s):
        """ms_audio_conference_remove_member: the pin unplumbed, its row cleared in every staging slot"""
        self.flags[s] = 0
        self.set_controls()
        self.held[:, s] = 0

    def join_seat(self, s, kind):
        """a NEW endpoint of `kind` on seat s, whoever held it: leave, then the pin plumbed with fresh MSVolume and resamplers at
        the new rate; the pin's input gain stays"""
        self.leave_seat(s)
        self.relabel(s, kind)
        self.flags[s] = L | A | O
        self.set_controls()
        self.restart(s)


def open_pair(br, ctx, mk, mm, conf, legs, admit):
    """the parts of an open bridge, their geometry checked against the bridge's"""
    parts = OpenParts(ctx, mk, mm, conf, legs, admit)
    assert br.tick_bytes() == (parts.in_pitch, parts.out_pitch)
    same_labels(br, parts)
    return parts


def same_labels(br, parts):
    """the bridge's host-side answers are the yardstick's labels"""
    for s in range(parts.n):
        assert br.leg_rate(s) == parts.rates[s] and br.leg_codec(s) == (parts.ic[s], parts.oc[s]), s
        assert br.leg_bytes(s) == (parts.in_bytes[s], parts.out_bytes[s]), s
    for c in range(parts.n // parts.mm):
        assert br.member_count(c) == int(((parts.flags[c * parts.mm:(c + 1) * parts.mm] & L) != 0).sum()), c


class OpenConcealedParts(_Seats, ConcealedParts):
    """ConcealedParts for the union: the decoders, a PlcBatch per admitted rate over all n rows, and a plc-less OPEN bridge
    (`inner`, itself held to OpenParts by the same test file) that takes the concealed PCM with every leg present"""

    def __init__(self, ctx, mk, mm, conf, legs, admit):
        kinds = union(legs, admit)
        widest = max(k[0] for k in kinds) // 100
        _Legs.__init__(self, ctx, legs, lambda _: widest)
        self.plc = {r: mk(ms.PlcBatch, self.n, r, max_block=self.width) for r in sorted(set(k[0] for k in kinds))}
        behind = lambda k: (k[0], PCM16, k[2])  # behind the concealer a leg's input is PCM
        self.inner = mk(ms.Bridge, self.n, members=mm, rate=conf, open=[behind(k) for k in legs], admit=[behind(k) for k in kinds])
        assert self.inner.tick_bytes()[0] == 2 * self.width
        self.t.cuda.synchronize()

    def join_seat(self, s, kind):
        self.relabel(s, kind)
        self.restart(s)  # the new endpoint's concealer starts from nothing
        self.inner.change(joins=[(s, (kind[0], PCM16, kind[2]))])

    def leave_seat(self, s):
        self.inner.change(leaves=[s])

