// tpe_pool.h — the host runtime's worker pool (tpe_pool.cpp) and the level
// packer's two steps (tpe_host.cpp), internal.
//
// The per-label host work of a suggest (the Parzen fits of every label a tree
// level needs, tpe.py:398-475 / 573-607 per label) is independent across
// labels; the reference does it one label at a time inside its pyll
// interpreter.  parallel_for runs such per-label jobs on a few resident worker
// threads plus the caller, so the host part of a suggest takes as long as its
// slowest label instead of the sum over labels.
#pragma once
#include <cstdint>

namespace tpe_pool {

// fn(ctx, i) for i in [0, n), on the caller and the pool's workers; returns
// when every call has returned.  Serial when the pool is off (tpe_host_threads
// 0), when n < 2, or when another thread holds the pool (nested or concurrent
// callers never wait on each other).
void parallel_for(int n, void (*fn)(void* ctx, int i), void* ctx);

// workers the next parallel_for may use (the caller not counted)
int workers();

// the process-wide device epoch (include/tpe_hip.h "Resident levels"): bumped
// by every exported entry that enqueues device work or packs into caller
// memory (returns the new epoch); a resident level of an older epoch is dead
uint64_t epoch_bump();
uint64_t epoch();

}  // namespace tpe_pool

// tpe_host_pack_level in its two steps (tpe_host.cpp; internal).  The plan
// validates the level, decides its tables and sort keys, sizes and places the
// blob's leading sections and — when the blob holds them (lead->direct) —
// writes the device-fit sections; it fills info's leading fields (the leading
// offsets, n_fit, fit_*, n_problems).  The fill writes everything else and the
// rest of info, with tpe_host_pack_level's return codes.  Between the two the
// caller may upload [0, lead->up_len) and launch the device fit, which touches
// the device blob's first lead->dev_bytes, so that it runs while the host fills
// the rest.  The level's state stays in per-thread scratch: the thread that
// planned calls the fill, with the same labels, blob and info.
struct tpe_label_in;
struct tpe_pack_info;
struct TpePackLead {
  int32_t direct;       // the leading sections landed in the blob
  int64_t up_len;       // the fit sections: blob bytes [0, up_len)
  int64_t dev_bytes;    // the device bytes the fit touches (through the patch rows)
};
extern "C" int tpe_internal_pack_plan(const struct tpe_label_in* labels, int32_t n_labels, int32_t n_cand,
                                      uint64_t seed, int64_t cand_base, int64_t n_cand_global, int32_t precision,
                                      void* blob, int64_t blob_cap, struct tpe_pack_info* info, TpePackLead* lead);
extern "C" int tpe_internal_pack_fill(struct tpe_pack_info* info);
