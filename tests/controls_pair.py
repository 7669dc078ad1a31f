"""What tests/test_gpu_bridge_controls.py and tests/test_gpu_session_controls.py share: a SUBJECT steered through
change_controls / change_members with three ticks in flight and observed through its reports, and a TWIN of the same build on
the same device that is fed the same input, driven by the waiting calls (set_controls, set_volume_params, remove_member /
add_member) one tick at a time and polled (active_speakers, levels) after every tick.  Everything the two produce is compared
bit for bit.  The pins' flags on the device have no read-out of their own; they are held through what they decide -- the
output rows (ACTIVE, OUTPUT, LINKED) and the device's election against the twin's roster (LINKED, ACTIVE)."""
import numpy as np

import mediastreamer2_amd as ms

L, A, O = ms.MI_MIX_LINKED, ms.MI_MIX_ACTIVE, ms.MI_MIX_OUTPUT
ON = L | A | O


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Pair:
    def __init__(self, subject, twin, fill, kinds=None):
        """fill(obj, t): acquire obj's staging and write tick t into it; kinds: a bridge's (rate, in_codec, out_codec) per seat"""
        self.b, self.a, self.fill, self.kinds = subject, twin, fill, kinds
        self.n, self.nconf = subject.n, subject.n // subject.members
        self.flags, self.gain = np.full(self.n, ON, np.uint8), np.ones(self.n, np.float32)
        self.got_b, self.got_a, self.reports, self.polls, self.maxima = [], [], [], [], []
        self.t = 0

    def close(self):
        self.b.close()
        self.a.close()

    # ---- one action on both sides
    def ctl(self, changes):
        """the subject through change_controls; the twin through the waiting setters"""
        self.b.change_controls(changes)
        self.mirror(changes)

    def mirror(self, changes):
        for s, f in changes:
            if "flags" in f:
                self.flags[s] = (self.flags[s] & L) | f["flags"]
            if "gain" in f:
                self.gain[s] = f["gain"]
            if "volume" in f:
                self.a.set_volume_params([f["volume"]], first=s)
        if any("flags" in f or "gain" in f for _, f in changes):
            self.a.set_controls(flags=self.flags, gain=self.gain)

    def members(self, joins=(), leaves=()):
        """the subject through change_members; the twin through remove_member / add_member (a JOIN on a taken seat replaces)"""
        if self.kinds is not None:
            self.b.change(joins=[(s, self.kinds[s]) for s in joins], leaves=list(leaves))
        else:
            self.b.change_members([(s, ms.MI_SESSION_LEAVE) for s in leaves] + [(s, ms.MI_SESSION_JOIN) for s in joins])
        self.members_waiting(self.a, joins, leaves)
        for s in leaves:
            self.flags[s] = 0
        for s in joins:
            self.flags[s] = ON

    def members_waiting(self, obj, joins=(), leaves=()):
        assert obj.in_flight() == 0 or obj is self.b
        for s in leaves:
            obj.remove_member(s)
        for s in joins:
            if self.flags[s] & L:
                obj.remove_member(s)
            obj.add_member(s)

    # ---- the ticks
    def _collect_b(self):
        self.got_b.append(self.b.collect().copy())
        try:
            r = self.b.collected_report()
            self.reports.append({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()})
        except ms.MiError:
            self.reports.append(None)

    def tick(self, full=(), filling=(), poll=False, state=None):
        """one tick on both.  full: actions made with three of the subject's ticks in flight and none collected; filling: between
        the subject's acquire and its submit.  Either way in_flight does not move across an action.  poll: the twin is polled
        after its tick.  state(subject, twin, t): a comparison made with the tick submitted on both"""
        b, a, t = self.b, self.a, self.t
        for act in full:
            assert b.in_flight() == 3
            act(self)
            assert b.in_flight() == 3
        if b.in_flight() == 3:
            self._collect_b()
        self.fill(b, t)
        for act in filling:
            k = b.in_flight()
            act(self)
            assert b.in_flight() == k
        b.submit()
        assert b.in_flight() == min(t + 1, 3)
        self.fill(a, t)
        a.submit()
        self.got_a.append(a.collect().copy())
        if poll:
            win, db = a.active_speakers(0)
            self.polls.append((win.copy(), db.copy(), a.levels().copy()))
            if hasattr(a, "volume_max"):
                self.maxima.append(a.volume_max().copy())
        if state:
            state(b, a, t)
        self.t += 1

    def drain(self):
        while self.b.in_flight():
            self._collect_b()

    def assert_same_rows(self, what=""):
        assert len(self.got_b) == len(self.got_a) == self.t
        for t, (x, y) in enumerate(zip(self.got_b, self.got_a)):
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: the rows of tick {t}")

    def assert_same_reports(self, first=0, what=""):
        """every collected tick's report against the twin's poll after the same tick: floats as words, winners as integers"""
        for t in range(first, self.t):
            r, (win, db, lev) = self.reports[t], self.polls[t]
            assert r is not None and r["seq"] == t, (what, t, r)
            np.testing.assert_array_equal(r["winner"], win, err_msg=f"{what}: winner of tick {t}")
            np.testing.assert_array_equal(words(r["max_db"]), words(db), err_msg=f"{what}: max_db of tick {t}")
            np.testing.assert_array_equal(words(r["levels"]), words(lev), err_msg=f"{what}: levels of tick {t}")


def ambiguous_maxima(maxima, flags_per_tick, members):
    """the ticks and conferences in which two eligible members' one-second maxima are DISTINCT floats whose dBm0 values are the
    same float -- where the report (the louder) and the reference (the earlier joiner) may differ.  maxima, flags: [ticks][n]"""
    bad = []
    for t, (mx, fl) in enumerate(zip(maxima, flags_per_tick)):
        with np.errstate(divide="ignore"):
            db = (np.float32(10) * np.log10(mx.astype(np.float32))).astype(np.float32)
        ok = ((fl & L) != 0) & ((fl & A) != 0) & (mx > 9e-4)  # (a superset of the eligible: -30 dBm0 is 1e-3)
        for c in range(len(mx) // members):
            idx = [i for i in range(c * members, (c + 1) * members) if ok[i]]
            for i in idx:
                for j in idx:
                    # (numpy's log10 need not round as libm's log10f does: anything within 8 ulp counts as well)
                    near = abs(int(words(mx[i:i + 1])[0]) - int(words(mx[j:j + 1])[0])) <= 8
                    if i < j and mx[i] != mx[j] and (db[i] == db[j] or near):
                        bad.append((t, c, i, j))
    return bad
