// Ensemble series (api_ensemble.inc): where member i's records of a series live inside that series' ONE device allocation.  Like
// frames.hpp and lines.hpp this header compiles for the host on its own -- it includes nothing of the project and no HIP -- so
// that the library and a stand-alone host program (tests/test_ensemble_slots_hostcheck.py) evaluate the very same lines.
//
// A series has one or more channels (the extrema: values, then cells), each a run of records per member.  Channel after channel,
// and within a channel member after member: member i's region of channel c holds cap[i] records of record_bytes[c][i] bytes.
//   film integrals   one channel, (FILM_NSUM + nsx_i + nsy_i) * 8 bytes per record, cap = LOG_CAPACITY / every + 1 for everyone
//   extrema          EXTREMA_NQ * 8 bytes (doubles), then EXTREMA_NQ * 2 * 4 bytes (int32), the same cap
//   probes           one channel, n_i * nv * 8 bytes per record, cap_i = the member's log capacity
// Nothing is padded: a channel of doubles starts on 8 bytes and one of int32 on 4 because every region before it is a whole number
// of doubles (hipMalloc's own alignment is far coarser).
#pragma once

#include <cstddef>
#include <vector>

namespace gpf {

struct EnsembleSlots {
    int m = 0;
    std::vector<size_t> off;    // [channel][member], in bytes from the allocation's start
    std::vector<size_t> bytes;  // [channel][member]: of one record
    size_t total = 0;           // bytes of the allocation
    int channels() const { return m > 0 ? (int)(off.size() / (size_t)m) : 0; }
    size_t at(int channel, int member) const { return off[(size_t)channel * (size_t)m + (size_t)member]; }
    size_t record_bytes(int channel, int member) const { return bytes[(size_t)channel * (size_t)m + (size_t)member]; }
};

// record_bytes[c][i]: bytes of one record of channel c of member i; cap[i]: records member i's regions hold
inline EnsembleSlots ensemble_slots(const std::vector<std::vector<size_t>>& record_bytes, const std::vector<long long>& cap) {
    EnsembleSlots s;
    s.m = (int)cap.size();
    for (const std::vector<size_t>& channel : record_bytes)
        for (int i = 0; i < s.m; ++i) {
            s.off.push_back(s.total);
            s.bytes.push_back(channel[(size_t)i]);
            s.total += (size_t)cap[(size_t)i] * channel[(size_t)i];
        }
    return s;
}

}  // namespace gpf
