// filters/conf_bank.inl -- a bank whose slots are CONFERENCES of `mm` members mixed on the device: what LegBank (leg_chain.inl:
// full sending legs) and ServerBank (server_leg.inl: a conference server's remote members) share.
// Part of the single translation unit filters.cpp (included inside its anonymous namespace, ahead of leg_chain.inl); not
// compiled on its own.
//
// One slot per MEMBER (conference * mm + pin).  The census (mixer_check_bypass, audiomixer.c:244-286), the channels' queues and
// their flow control (:92-111) run on COUNTS on the host; the mixer's controls, MSVolume's parameters and running state, the
// meters' read-back and the pinned slab the mixes come back in live here once; the early launch at the end of the graph walk is
// EarlyBank's (round_bank.inl), counted per conference (conf_walked).
// What differs between the two banks is reached through hooks: enqueue_at (the bank's launches), slab_bytes, the members' own
// delivered() / has_staged() / prefetch_meters(), and the few overrides that say so.

constexpr int kLegMeterRounds = 8; // rounds before the last of a flush whose meter state is read back (kLegLightRounds, kLegMaxChunks fit)

struct MixSlab { // one flush's conference mixes in pinned memory, referenced by the blocks handed downstream
	std::atomic<int> state{0}; // 0 free, 1 a data block is alive on it, 2 its bank is gone (freed when the block goes)
	size_t bytes = 0;
	uint8_t *payload() { return reinterpret_cast<uint8_t *>(this) + 64; }
	static MixSlab *of(void *payload) { return reinterpret_cast<MixSlab *>(static_cast<uint8_t *>(payload) - 64); }
};
static_assert(sizeof(MixSlab) <= 64, "slab header");
void mix_slab_release(void *payload) { // db_freefn of the slab's data block (the last dupb of a flush was freed)
	MixSlab *s = MixSlab::of(payload);
	if (s->state.exchange(0, std::memory_order_acq_rel) == 2) mi_host_free(nullptr, s);
}

int channel_flow_control_level(Channel *chan, int level, int threshold, uint64_t now); // mixer.inl

// a member of such a conference, as the counting sees it (FusedLeg and ServerLeg derive from it)
struct ConfMember {
	int slot = 0, pin = 0;
	uint32_t lv_from = 0; // MSMI355X_CHECK_LEVELS: the first read-back of the queues' levels (ConfBank::lv_seq) that is this member's -- an earlier one shows the slot before it was taken
	MSFilter *vol = nullptr, *mixer = nullptr;
	int new_samples = 0;  // samples MSVolume put on the mixer's queue since the mixer last looked
	int chan_samples = 0; // the mixer channel's bufferizer, samples (what f_chan holds)
	bool metered = false;
};

// Leg: the bank's member type, derived from ConfMember, with
//   bool delivered() const     -- it has put something on its mixer pin's queue since the mixer last looked
//   bool has_staged() const    -- it has staged rows whose launches have not left
//   static void prefetch_meters(Leg *const *legs, size_t s, size_t n)   -- read_meters()'s walk over legs[0, n) is at s
template <class Leg>
struct ConfBank : EarlyBank<Pool> {
	int mm = 0, ns = 0, nlegs = 0;
	mi_volume *vol = nullptr, *vol_id = nullptr; // vol_id: identity batch (gain 1, nothing enabled): volmix_kernel's volume half for a levelled queue
	mi_fifo *f_chan = nullptr;                   // the mixer channels' bufferizers, where they hold levelled samples
	mi_mixer *mix = nullptr;
	int16_t *d_mix = nullptr, *d_scratch = nullptr; // [capacity][mm][ns]; [nlegs][ns]
	uint8_t *h_run = nullptr, *d_run = nullptr;     // [capacity]: conferences that tick in this launch of the volume + mix kernel
	uint8_t *h_dgate = nullptr, *d_dgate = nullptr; // [nlegs]: the leg the channels' flow control drops samples of (rare)
	mi_volume_state *h_vstate = nullptr;            // pinned [nlegs]
	// MSVolume records EVERY chunk's energy in its extrema (update_energy, msvolume.c:405-406): when a flush levels more than one
	// chunk of a leg, the state behind each round but the last comes back too (kLegMeterRounds rows of [nlegs]; vhas: the leg had a
	// chunk in that round)
	mi_volume_state *h_vround = nullptr;
	std::vector<uint8_t> vhas;
	int vrounds = 0;
	int16_t *h_copy = nullptr;  // the mixes when every slab is still held downstream: emitted by copy
	std::vector<MixSlab *> slabs;
	MixSlab *cur = nullptr;     // the slab this flush downloads into (null: h_copy)
	mblk_t *root = nullptr;     // its data block, alive from finish() to emitted()
	std::vector<Leg *> legs;
	std::vector<uint8_t> conf_ready;
	std::vector<int> lone; // the single contributor's pin of a conference that ticked with one, else -1
	std::vector<uint8_t> flags;
	std::vector<float> gains;
	bool ctl_dirty = true;
	// what a method set while the last walk's blocks were still waiting for the coming flush (Pool::work_waiting): live when that flush is
	// through (flushed()).  vp_dirty / vs_dirty: 1 = goes to the device with the next enqueue, 2 = waits for flushed() first
	std::vector<uint8_t> next_flags, next_conf;
	std::vector<float> next_gains;
	bool next_any = false;
	std::vector<mi_volume_params> vparams;
	std::vector<mi_volume_state> vstate;
	std::vector<uint8_t> vp_dirty, vs_dirty;
	bool v_dirty = false;
	struct GainPatch {
		float gain, target;
		bool also_target;
	};
	std::vector<GainPatch> vpatch; // MS_VOLUME_SET_GAIN & co. on a fused leg: the two fields, set on the state as the device holds it
	std::vector<std::pair<int, int>> sdrops; // (leg slot, samples) the mixer channels' flow control discards this flush
	std::vector<uint64_t> conf_time;         // ticker time of a conference's last tick (one per tick, whoever enqueues)
	std::vector<uint32_t> walk_tick;         // ticker tick in which a conference's mixer was last walked
	// The staging rows and the mixes' slab are pinned host memory the device addresses itself: by default the launches read
	// and write them where they lie (a few hundred bytes per leg, once) and the tick path makes no copy at all -- four
	// launches and the meters' read-back.  MSMI355X_ZERO_COPY=0: staged through device buffers by copy launches (A/B).
	bool zero_copy = true;
	bool mixed = false, check_levels = false, lv_fresh = false;
	uint32_t lv_seq = 0; // read-backs of the levels so far (ConfMember::lv_from)

	explicit ConfBank(int members) : mm(members) {}
	// the host's rows, once the derived constructor knows capacity and nlegs (the device's and the pinned ones are the derived bank's to size)
	void init_conf() {
		const size_t L = (size_t)nlegs;
		vhas.assign((size_t)kLegMeterRounds * L, 0);
		conf_time.assign((size_t)capacity, (uint64_t)-1);
		walk_tick.assign((size_t)capacity, 0);
		legs.assign(L, nullptr);
		conf_ready.assign((size_t)capacity, 0);
		lone.assign((size_t)capacity, -1);
		flags.assign(L, 0);
		gains.assign(L, 1.0f);
		next_flags.assign(L, 0);
		next_gains.assign(L, 1.0f);
		next_conf.assign((size_t)capacity, 0);
		mi_volume_params p;
		mi_volume_default_params(&p);
		vparams.assign(L, p);
		vstate.resize(L);
		vp_dirty.assign(L, 0);
		vs_dirty.assign(L, 0);
		vpatch.assign(L, GainPatch{1.f, 1.f, false});
		check_levels = getenv("MSMI355X_CHECK_LEVELS") != nullptr;
		zero_copy = zero_copy_rows();
	}
	~ConfBank() override { // (behind the derived bank's: the stream has been waited for, the batch objects are gone)
		if (root) freeb(root);
		for (Leg *l : legs) delete l;
		for (MixSlab *s : slabs) // a slab whose blocks are still held downstream outlives the bank: its last block frees it
			if (s->state.exchange(2, std::memory_order_acq_rel) == 0) mi_host_free(hub->ctx, s);
	}

	// (enqueue_at(now), EarlyBank's hook: the bank's uploads and launches for everything staged, the conferences ticking at `now`)
	virtual size_t slab_bytes() const = 0;     // what one flush downloads into a slab

	MixSlab *free_slab() {
		for (MixSlab *s : slabs)
			if (s->state.load(std::memory_order_acquire) == 0) return s;
		if (slabs.size() >= 4 || failed) return nullptr;
		const size_t bytes = slab_bytes();
		void *p = mi_host_alloc(hub->ctx, 64 + bytes);
		if (!p) return nullptr;
		MixSlab *s = new (p) MixSlab();
		s->bytes = bytes;
		slabs.push_back(s);
		return s;
	}
	// this flush's slab goes downstream: its data block, which the rows handed on refer to (row_block)
	void slab_out() {
		cur->state.store(1, std::memory_order_release);
		root = esballoc(cur->payload(), cur->bytes, 0, mix_slab_release);
	}
	// `n` samples at sample `at` of this flush's results as a block: the row as it lies in the slab, or a copy when every slab was still held downstream
	mblk_t *row_block(size_t at, int n) {
		uint8_t *row = (root ? cur->payload() : reinterpret_cast<uint8_t *>(h_copy)) + at * 2;
		mblk_t *om;
		if (root) {
			om = dupb(root);
			om->b_rptr = row;
			om->b_wptr = row + (size_t)n * 2;
		} else {
			om = allocb((size_t)n * 2, 0);
			memcpy(om->b_wptr, row, (size_t)n * 2);
			om->b_wptr += n * 2;
		}
		return om;
	}
	void emitted() override { // the flush's own reference: the slab returns to the ring when the last block downstream is freed
		if (root) freeb(root);
		root = nullptr;
		cur = nullptr;
	}

	// ---- one tick of a conference on counts: mixer_process (audiomixer.c:288-346) with the census of mixer_check_bypass
	// (:244-286) and the channels' flow control (:92-111), deciding from what MSVolume would have put on the pins' queues
	void conf_tick(int c, uint64_t now) {
		MSFilter *mx = owner[(size_t)c];
		MixerState *s = (MixerState *)mx->data;
		conf_ready[(size_t)c] = 0;
		lone[(size_t)c] = -1;
		int count = 0, who = -1;
		for (int pin = 0; pin < mm; ++pin) {
			Leg *leg = legs[(size_t)(c * mm + pin)];
			if (!leg) continue;
			uint64_t &seen = s->channels[pin].last_activity;
			bool contributes;
			if (leg->delivered()) {
				seen = now;
				contributes = true;
			} else if (seen == (uint64_t)-1) {
				seen = now; // first look at a silent pin only starts its clock
				contributes = false;
			} else {
				contributes = now - seen < BYPASS_MODE_TIMEOUT;
			}
			if (contributes) ++count, who = pin;
		}
		if (count == 0) return; // nobody has delivered for a second: nothing leaves (and nothing was queued)
		if ((count == 1) != (s->bypass_mode != FALSE))
			ms_message("mi355x mixer %p: %s", (void *)mx, count == 1 ? "a single contributor (mixed on the device all the same)" : "two or more contributors");
		s->bypass_mode = count == 1;
		channels_tick(c, s, now);
		conf_ready[(size_t)c] = 1;
		lone[(size_t)c] = count == 1 ? who : -1;
	}
	// the channels' half of that tick.  Here: the channel's bufferizer holds levelled samples, the tick reads 10 ms of them or nothing (:78-90)
	virtual void channels_tick(int c, MixerState *s, uint64_t now) {
		for (int pin = 0; pin < mm; ++pin) {
			Leg *leg = legs[(size_t)(c * mm + pin)];
			if (!leg) continue;
			leg->chan_samples += leg->new_samples;
			leg->new_samples = 0;
			if (leg->chan_samples >= ns) leg->chan_samples -= ns;
			const int skip = channel_flow_control_level(&s->channels[pin], leg->chan_samples * 2, s->skip_threshold, now);
			if (skip > 0) {
				const int k = std::min(leg->chan_samples, skip / 2);
				ms_warning("mi355x mixer: pin %i kept more than two ticks queued for 5 s; %i samples discarded", pin, k);
				leg->chan_samples -= k;
				if (k > 0) sdrops.push_back({leg->slot, k});
			}
		}
	}
	// ... and on the device: the samples that flow control discards (rare: a pin that kept two ticks queued for 5 s)
	void discard_sdrops() {
		const size_t L = (size_t)nlegs;
		for (const auto &dk : sdrops) {
			memset(h_dgate, 0, L);
			h_dgate[(size_t)dk.first] = 1;
			if (!zero_copy) MI_MUST(mi_copy_h2d_pinned(hub->ctx, d_dgate, h_dgate, L));
			for (int left = dk.second; left > 0; left -= std::min(left, ns))
				MI_MUST(mi_fifo_pop(f_chan, std::min(left, ns), d_scratch, ns, nullptr, zero_copy ? h_dgate : d_dgate, 0));
			sync_stream(); // (the gate row is rewritten for the next one)
		}
	}

	// A conference with a SINGLE contributor is in the reference's bypass mode (audiomixer.c:219-286): that pin's blocks go to the other
	// outputs AS THEY ARE -- no input gain, no regard for MS_AUDIO_MIXER_SET_ACTIVE (mixer_dispatch_output never looks at the channel).
	// The batch mixes such a conference all the same, with that pin's controls set to "active, gain 1" for as long as it is alone:
	// the sum of one is the block itself (but for a sample of -32768, which the sum saturates to -32767: the stated exception).
	std::vector<int> lone_ctl;           // per conference: the pin whose controls are overridden right now, -1 = none
	std::vector<uint8_t> eff_flags;
	std::vector<float> eff_gains;
	void push_controls() {
		if (!mix) return;
		bool moved = false;
		if (lone_ctl.size() != lone.size()) lone_ctl.assign(lone.size(), -1), moved = true;
		for (size_t c = 0; c < lone.size(); ++c) {
			if (!owner[c] && lone_ctl[c] >= 0) lone_ctl[c] = -1, moved = true; // (the slot was given up)
			if (owner[c] && conf_ready[c] && lone_ctl[c] != lone[c]) lone_ctl[c] = lone[c], moved = true; // (a conference that does not tick keeps what it had)
		}
		if (!ctl_dirty && !moved) return;
		eff_flags = flags, eff_gains = gains;
		for (size_t c = 0; c < lone_ctl.size(); ++c)
			if (lone_ctl[c] >= 0) {
				const size_t at = c * (size_t)mm + (size_t)lone_ctl[c];
				eff_flags[at] |= MI_MIX_ACTIVE;
				eff_gains[at] = 1.0f;
			}
		MI_MUST(mi_mixer_set_controls(mix, eff_flags.data(), eff_gains.data()));
		ctl_dirty = false;
	}
	// MS_AUDIO_MIXER_SET_INPUT_GAIN / SET_ACTIVE / ENABLE_OUTPUT on the conference in slot c (hub locked): the bank's control rows
	void push_mixer_controls(MSFilter *f, MixerState *s, int c, bool from_method) {
		const bool later = from_method && work_waiting();
		std::vector<uint8_t> &fl_row = later ? next_flags : flags;
		std::vector<float> &g_row = later ? next_gains : gains;
		for (int pin = 0; pin < mm; ++pin) {
			const size_t at = (size_t)(c * mm + pin);
			uint8_t fl = 0;
			if (f->inputs[pin] && legs[at]) fl |= MI_MIX_LINKED;
			if (s->channels[pin].active) fl |= MI_MIX_ACTIVE;
			if (f->outputs[pin] && s->channels[pin].output_enabled) fl |= MI_MIX_OUTPUT;
			fl_row[at] = fl;
			g_row[at] = s->channels[pin].gain;
		}
		if (later) next_conf[(size_t)c] = 1, next_any = true;
		else next_conf[(size_t)c] = 0, ctl_dirty = true;
	}
	// the coming flush is through: the controls the methods set while its blocks were waiting go live (the tail of the banks' flushed())
	void controls_flushed() {
		if (!next_any) return;
		for (int c = 0; c < hi; ++c) {
			if (!next_conf[(size_t)c]) continue;
			const size_t at = (size_t)c * mm;
			std::copy(next_flags.begin() + at, next_flags.begin() + at + mm, flags.begin() + at);
			std::copy(next_gains.begin() + at, next_gains.begin() + at + mm, gains.begin() + at);
			next_conf[(size_t)c] = 0;
			ctl_dirty = true;
		}
		next_any = false;
	}
	// MS_VOLUME_* methods on member s's MSVolume (hub locked): parameters / running state for the next flush.  Returns when they go:
	// 1 with the next enqueue, 2 behind the coming flush (flushed())
	uint8_t push_volume(size_t s, const mi_volume_params *p, int peer, const float *gain, const float *target) {
		const uint8_t when = work_waiting() ? 2 : 1;
		vparams[s] = *p;
		vparams[s].peer = peer;
		vp_dirty[s] = when;
		if (gain) {
			vpatch[s] = {*gain, target ? *target : 0.f, target != nullptr};
			vs_dirty[s] = when;
		}
		v_dirty = true;
		return when;
	}

	// the meters behind a levelling round that is not the flush's last (read back with the round's results: read_meters() records them)
	void meter_round(size_t UL) {
		if (vrounds >= kLegMeterRounds || failed) return;
		MI_MUST(mi_volume_get_state_async(vol, 0, (int)UL, h_vround + (size_t)vrounds * nlegs));
		++vrounds;
	}
	// finish(), when something was levelled: MSVolume's running state as the device left it, and its extremum records
	void read_meters() {
		const size_t L = (size_t)nlegs, UL = (size_t)hi * mm;
		for (size_t s = 0; s < UL; ++s) {
			Leg *leg = legs[s];
			Leg::prefetch_meters(legs.data(), s, UL);
			if (!leg) continue;
			vstate[s] = h_vstate[s];
			if (leg->metered && hub->ticker) { // update_energy's extremum records, msvolume.c:405-406: one per chunk or block, in order
				VolumeData *vd = (VolumeData *)leg->vol->data;
				for (int r = 0; r < vrounds; ++r)
					if (vhas[(size_t)r * L + s]) {
						vd->max.record_max(hub_time(hub), h_vround[(size_t)r * L + s].energy);
						vd->min.record_min(hub_time(hub), h_vround[(size_t)r * L + s].energy);
					}
				vd->max.record_max(hub_time(hub), vstate[s].energy);
				vd->min.record_min(hub_time(hub), vstate[s].energy);
			}
			leg->metered = false;
		}
		std::fill(vhas.begin(), vhas.end(), 0);
		vrounds = 0;
	}

	// a conference's mixer runs behind all of its members: the last conference of the bank to be walked sends the bank's work off
	void conf_walked(int c) {
		if (!walk_begins()) return;
		if (walk_tick[(size_t)c] == hub->ticker->ticks) return;
		walk_tick[(size_t)c] = hub->ticker->ticks;
		walk_counted();
	}
	// A slot's owner leaves while the bank's work for the coming tick is already out (it left at the end of the last graph walk):
	// the reference's filters would have handed that tick's audio on in the walk itself, so it goes out now -- the owner's own
	// mix or chunks; the others' follow with the hub's flush as usual.
	void deliver_in_flight(MSFilter *owner_filter, int slot) {
		if (failed || (!outstanding && !early)) return;
		sync_stream();
		if (failed) return;
		outstanding = false;
		deliver_now(owner_filter, slot);
	}
	virtual void deliver_now(MSFilter *owner_filter, int slot) = 0; // finish() and emit() for that slot (the two banks differ in what they hand on: see their overrides)
	// vstate as the device holds it NOW (a member is about to leave with its MSVolume's running state): launches that are out and not
	// waited for yet are waited for, their read-back taken
	void settle_meters() {
		if (!outstanding && !early) return;
		if (failed) return;
		sync_stream();
		if (failed || !meters_came_back()) return;
		for (size_t s = 0; s < (size_t)nlegs; ++s)
			if (legs[s] && !vs_dirty[s]) vstate[s] = h_vstate[s];
	}
	virtual bool meters_came_back() const = 0; // (the two banks differ: see their overrides)
	// A graph is being detached (facade_detached, filters.cpp): its fused conferences' and legs' tick in flight is waited for and handed
	// on -- speaker frames, mixes / chunks -- before any of its facades lets go (the scoped flush then carries those blocks on through
	// whatever facades of the graph sit behind: an encoder, a resampler)
	void deliver_in_scope() {
		// (a launch is the whole bank's: it leaves from here -- possibly the application's thread, in the middle of the ticker's walk of the bank's
		// OTHER graphs, with only part of them staged -- only when the detaching graph itself staged something that has not left; between two ticks
		// its work is out already and there is nothing to launch)
		const auto in_scope = [&](int s) { return owner[(size_t)s] && hub->scope->count(owner[(size_t)s]); };
		bool ours = false;
		for (int s = 0; s < hi && !ours; ++s) {
			if (!in_scope(s)) continue;
			for (int pin = 0; pin < mm && !ours; ++pin)
				if (const Leg *leg = legs[(size_t)(s * mm + pin)]) ours = leg->has_staged();
		}
		if (ours) launch_staged();
		for (int s = 0; s < hi; ++s)
			if (in_scope(s)) deliver_in_flight(owner[(size_t)s], s);
	}
};
// the banks of one kind (their keys' prefix) among a hub's, in the hub's order
template <class Bank>
void deliver_banks_in_scope(TickerHub &h, const char *prefix) {
	for (Pool *p : h.pools)
		if (p->key.compare(0, strlen(prefix), prefix) == 0) static_cast<Bank *>(p)->deliver_in_scope();
}
