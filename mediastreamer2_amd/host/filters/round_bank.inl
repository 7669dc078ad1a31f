// filters/round_bank.inl -- what the banks share between Pool and their own launches, each written once:
//   RoundBank     a per-stream bank that launches in ROUNDS (a stream's k-th block of the tick goes out in round k): who staged how
//                 much, the pinned length (and mode) rows with their scoped copy, the settle step of finish()
//   DropRequests  MS_AUDIO_FLOW_CONTROL_DROP requests on their way to an mi_flowctl batch (FlowPool, RecvBank)
//   EarlyBank     a fused bank whose launches leave at the END of the graph walk instead of with the next tick's flush
//                 (ConfBank<Leg>, RecvBank)
// Part of the single translation unit filters.cpp (included inside its anonymous namespace, ahead of the facades); not compiled on
// its own.

struct RoundBank : Pool {
	std::vector<int> staged, ready; // blocks (EcPool: frames) a slot has staged since the last launch / has had launched, to be emitted
	// [kMaxRounds][capacity] pinned: samples per round and slot.  h_lensc: the same rows while a detaching graph's slots alone are
	// flushed (TickerHub::scope) -- everybody else counts as empty in THAT launch and keeps what it staged in h_len.  d_len:
	// [capacity], for the banks that stage through device buffers (always, or with MSMI355X_ZERO_COPY=0)
	int32_t *h_len = nullptr, *h_lensc = nullptr, *d_len = nullptr;
	uint8_t *h_mode = nullptr, *h_modesc = nullptr, *d_mode = nullptr; // a second row (MI_PLC_*) through the same masking: PlcPool, RecvBank
	// (behind Building, once the capacity is known.  rows = false: staged / ready alone, for a bank whose launch takes another kind of row)
	void init_rounds(bool rows = true, bool modes = false) {
		const size_t c = (size_t)capacity;
		staged.assign(c, 0);
		ready.assign(c, 0);
		if (!rows) return;
		h_len = pinned<int32_t>(kMaxRounds * c);
		h_lensc = pinned<int32_t>(kMaxRounds * c);
		d_len = devmem<int32_t>(c);
		if (!modes) return;
		h_mode = pinned<uint8_t>(kMaxRounds * c);
		h_modesc = pinned<uint8_t>(kMaxRounds * c);
		d_mode = devmem<uint8_t>(c);
	}
	int rounds() const { // what this flush launches: the most any slot that takes part has staged
		int maxr = 0;
		for (int s = 0; s < hi; ++s)
			if (!parked(s)) maxr = std::max(maxr, staged[(size_t)s]);
		return maxr;
	}
	// The length row the launch of round r is to be given: slots that staged fewer than r + 1 blocks count as empty.  With the whole
	// bank flushing they are zeroed in place; while a detaching graph's slots alone are flushed the launch gets a masked COPY.  The
	// mode row goes through the same step (mode_row(r), afterwards)
	const int32_t *len_row(int r) {
		const size_t c = (size_t)capacity;
		int32_t *len = h_len + (size_t)r * c;
		uint8_t *mode = h_mode ? h_mode + (size_t)r * c : nullptr;
		if (!hub->scope) {
			for (size_t s = 0; s < c; ++s)
				if (staged[s] <= r) { // (slots beyond `hi` have never staged)
					len[s] = 0;
					if (mode) mode[s] = MI_PLC_NONE;
				}
			return len;
		}
		int32_t *lsc = h_lensc + (size_t)r * c;
		for (size_t s = 0; s < c; ++s) {
			const bool in = (int)s < hi && staged[s] > r && !parked((int)s);
			lsc[s] = in ? len[s] : 0;
			if (mode) h_modesc[(size_t)r * c + s] = in ? mode[s] : (uint8_t)MI_PLC_NONE;
		}
		return lsc;
	}
	const uint8_t *mode_row(int r) const { return (hub->scope ? h_modesc : h_mode) + (size_t)r * capacity; }
	// ... and through the device's copy of a row, for a launch that does not read pinned memory
	const int32_t *on_device(const int32_t *len) {
		MI_MUST(mi_copy_h2d_pinned(hub->ctx, d_len, len, (size_t)capacity * 4));
		return d_len;
	}
	const uint8_t *on_device(const uint8_t *mode) {
		MI_MUST(mi_copy_h2d_pinned(hub->ctx, d_mode, mode, (size_t)capacity));
		return d_mode;
	}
	// finish(): what was staged has been launched and is the slots' to emit (deliver = false: nothing is)
	void settle(bool deliver = true) {
		for (int s = 0; s < hi; ++s) {
			if (parked(s)) continue;
			ready[(size_t)s] = deliver ? staged[(size_t)s] : 0;
			staged[(size_t)s] = 0;
		}
	}
	bool scoped() const override { return true; } // (everything above asks parked())
};

// MS_AUDIO_FLOW_CONTROL_DROP (flowcontrol.c:199-211) takes effect exactly where it fell in the stream's block sequence: before round r
// for a request that r staged blocks preceded.  A stream that is still dropping ignores its request on the device, like :204 does.
struct DropRequests {
	std::vector<uint32_t> req_drop, req_total, arm_drop, arm_total; // pending per slot; the rows the device is handed (arm)
	std::vector<int> req_round;                                     // staged blocks of the stream that precede its request
	bool have_req = false;
	void init(size_t c) {
		req_drop.assign(c, 0), req_total.assign(c, 0), arm_drop.assign(c, 0), arm_total.assign(c, 0);
		req_round.assign(c, 0);
	}
	// the event in samples (:201-203)
	static uint32_t samples(uint32_t ms, int rate, int nchannels) { return (ms * (uint32_t)rate * (uint32_t)nchannels) / 1000; }
	bool pending(size_t s) const { return req_drop[s] != 0 || req_total[s] != 0; }
	void request(size_t s, uint32_t drop, uint32_t total, int rounds_staged) {
		if (pending(s)) return; // (ignored while one is pending, like :204)
		req_drop[s] = drop, req_total[s] = total;
		req_round[s] = rounds_staged;
		have_req = true;
	}
	void forget(size_t s) { req_drop[s] = req_total[s] = 0; }
	void clear() { // a broken context drops nothing
		have_req = false;
		std::fill(req_drop.begin(), req_drop.end(), 0u);
		std::fill(req_total.begin(), req_total.end(), 0u);
	}
	// the requests that fell before round r of their stream (last: everything left) go to the device
	void arm(Pool &bank, mi_flowctl *fc, int r, bool last) {
		if (!have_req || !fc) return;
		bool any = false, left = false;
		for (int s = 0; s < bank.capacity; ++s) {
			arm_drop[(size_t)s] = arm_total[(size_t)s] = 0;
			if (!pending((size_t)s)) continue;
			if (s < bank.hi && bank.parked(s)) { // (not this flush's business: the request waits for the slot's own)
				left = true;
				continue;
			}
			if (last || req_round[(size_t)s] <= r) {
				arm_drop[(size_t)s] = req_drop[(size_t)s], arm_total[(size_t)s] = req_total[(size_t)s];
				forget((size_t)s);
				any = true;
			} else left = true;
		}
		if (any && mi_flowctl_request_drop(fc, arm_drop.data(), arm_total.data()) != MI_OK) bank.failed = mi_failed("mi_flowctl_request_drop");
		have_req = left;
	}
};

// Everything a tick will stage IS staged when the last of the bank's slots has been walked (the filter that is counted runs behind
// the others of its slot in the ticker's depth-first order, msticker.c:261-282): the bank's uploads and launches go out THEN, at the
// end of the graph walk, instead of at the start of the next tick -- the device works through the idle part of the interval and the
// next tick's flush finds the results waiting.  Same results, same one tick of latency; the launches just leave the tick's critical
// path.  (A tick in which some slot was not walked falls back to the flush.)  Base: Pool for ConfBank, RoundBank for RecvBank.
template <class Base>
struct EarlyBank : Base {
	bool staged_since = false;             // something was staged (or a slot joined) since the last enqueue
	bool outstanding = false;              // an enqueue has not been waited for yet
	bool early = false, early_any = false; // this tick's work was enqueued at the end of the walk; ... and it enqueued something
	bool no_early = getenv("MSMI355X_NO_EARLY_LAUNCH") != nullptr; // A/B switch: everything leaves at the flush
	int walked = 0;                        // slots that have been walked in this tick's graph walk
	uint32_t walk_epoch = 0;
	uint64_t launches = 0;
	// the bank's uploads and launches for everything staged, its mixers' clock (if it has any) reading `now`; true: something left
	virtual bool enqueue_at(uint64_t now) = 0;
	bool enqueue() override {
		bool any = false;
		const bool was_early = early;
		if (early) { // already out since the end of the last graph walk
			early = false;
			any = early_any;
		}
		// (what was staged after an early launch -- a slot that joined the bank later in that walk, a PLC run by the flush -- goes out now)
		if (!was_early || staged_since) any |= enqueue_at(hub_time(this->hub));
		outstanding = false; // the hub waits for the stream right behind this
		return any;
	}
	// A slot is being walked.  false: no early launch (switched off, this tick's has left already -- or, for a bank that says so, the
	// hub's flush is what runs the filter).  The caller then sees that the slot is counted once per tick and calls walk_counted()
	bool walk_begins(bool also_in_flush = true) {
		if (no_early || this->failed || early || !this->hub->ticker || (!also_in_flush && this->hub->in_flush)) return false;
		const uint32_t tick = this->hub->ticker->ticks;
		if (walk_epoch != tick) walk_epoch = tick, walked = 0;
		return true;
	}
	void walk_counted() { // one more of the bank's slots has been walked in this tick: the last one launches
		if (++walked < this->in_use) return;
		early_any = enqueue_at(hub_time(this->hub) + (uint64_t)this->hub->ticker->interval); // the clock reads what the flush would
		early = true;
	}
	// a graph is being detached between two ticks: rows staged in the last walk whose launches have not left -- a bank without early
	// launch, a slot that joined the bank mid-walk -- leave now, as the coming flush would send them (the walks are over and the
	// ticker's clock reads what that flush would read): the tick in flight includes them
	void launch_staged(bool without_ticker = false) {
		if (this->failed || !staged_since || !(this->hub->ticker || without_ticker)) return;
		const bool more = enqueue_at(hub_time(this->hub));
		early_any = early ? (early_any || more) : more;
		early = true;
	}
};
