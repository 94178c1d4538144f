// Which record launches land on record slots of a trace arena's kept regions (h2r_arena_create): pure host code, no HIP, so that
// tests/cpp/test_arena_match.cpp can run it without a device.
//
// The constant planes of a record (ACCX_LO/HI, QACC, MODACC, NQ2_LO/HI, AMNQ2: the acc_extra chain of is_equal_muled) depend on
// (limb width, limbs) alone.  The arena's look writes them into every record slot of every region it keeps, so a launch whose
// records ALL lie on such slots may leave them alone (TraceArgs::keep_const).  The match is exact: anything that is not provably a
// set of whole record slots of one registered region writes complete records.
#pragma once
#include <cstdint>
#include <mutex>
#include <vector>

namespace h2r_arena_match {

// The geometry an arena was created for, and one of its kept regions.
struct Region {
    int device = 0;
    uint32_t limb_width = 0, num_limbs = 0;
    uint64_t base = 0, bytes = 0;               // bytes = batch * elem_stride
    uint64_t elem_stride = 0, first_record_off = 0;
    uint32_t records_per_elem = 0;
    uint64_t batch = 0;
    const void *owner = nullptr;                // the arena (unregister_owner)
};

// The records of one launch: element e in [0, elems), record t in [t_lo, t_lo + T) at trace + e * elem_stride + off_records + t * record_stride.
struct Launch {
    int device = 0;
    uint32_t limb_width = 0, num_limbs = 0;
    uint64_t trace = 0;
    uint64_t elem_stride = 0, off_records = 0;
    uint32_t t_lo = 0, T = 0;
    uint64_t elems = 0;
};

inline bool covers(const Region &r, const Launch &l) {
    if (!r.base || !l.trace || !l.elems || !l.T || !r.elem_stride) return false;
    if (l.device != r.device || l.limb_width != r.limb_width || l.num_limbs != r.num_limbs) return false;
    if (l.elem_stride != r.elem_stride || l.off_records != r.first_record_off) return false;
    if (l.trace < r.base || l.trace - r.base >= r.bytes) return false;
    const uint64_t d = l.trace - r.base;
    if (d % r.elem_stride) return false;
    const uint64_t first = d / r.elem_stride;
    if (l.elems > r.batch || first > r.batch - l.elems) return false;
    return (uint64_t)l.t_lo + l.T <= r.records_per_elem;
}

class Registry {
public:
    void add(const Region &r) { std::lock_guard<std::mutex> lk(mu_); regions_.push_back(r); }
    void unregister_owner(const void *owner) {
        std::lock_guard<std::mutex> lk(mu_);
        for (size_t i = regions_.size(); i-- > 0;)
            if (regions_[i].owner == owner) regions_.erase(regions_.begin() + (long)i);
    }
    bool match(const Launch &l) const {
        std::lock_guard<std::mutex> lk(mu_);
        for (const Region &r : regions_) if (covers(r, l)) return true;
        return false;
    }
    size_t size() const { std::lock_guard<std::mutex> lk(mu_); return regions_.size(); }
private:
    mutable std::mutex mu_;
    std::vector<Region> regions_;
};

}  // namespace h2r_arena_match
