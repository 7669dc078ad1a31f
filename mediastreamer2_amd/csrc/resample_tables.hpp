// resample_tables.hpp -- the tables of the one-member-per-wavefront resamplers (bridge_phases.hpp), built on the host from
// mi_resampler's own design code: what bridge.hip's build_tables and session_legs.hip's share.
#pragma once
#include "common.hpp"

#include <vector>

namespace {

// the polyphase table of mi_resampler's own design code (quality 3, what msresample.c uses) for in_rate -> out_rate
// filt_len, direct: mi_resampler_info's verdict on that design
inline int design_table(mi_ctx *ctx, int in_rate, int out_rate, std::vector<float> &table, int *filt_len = nullptr, int *direct = nullptr) {
	mi_resampler *r = nullptr;
	int rc = mi_resampler_create(ctx, 1, (uint32_t)in_rate, (uint32_t)out_rate, 3, &r);
	if (rc != MI_OK) return rc;
	table.resize((size_t)mi_resampler_get_table(r, nullptr, 0));
	mi_resampler_get_table(r, table.data(), (int)table.size());
	rc = mi_resampler_info(r, filt_len, nullptr, nullptr, direct);
	mi_resampler_destroy(r);
	return rc;
}

// a down-sampler by m as resample_down's lanes read it: the designed [1][taps * m] row phase-major, tap m * i + p at [p][i]
inline void append_phase_major(std::vector<float> &all, const std::vector<float> &t, int m, int taps) {
	for (int p = 0; p < m; ++p)
		for (int i = 0; i < taps; ++i) all.push_back(t[(size_t)i * m + p]);
}

} // namespace
