// The TCP session machine on the host: ppe_stream_step (csrc/ppe_stream_session_dev.h), the function the session kernel
// compiles, behind a C entry point with no context and no device.  The CPU tests hold it against the serial model
// (tests/stream_session_model.py) packet by packet, so the function the GPU runs is checked where no GPU is.
#include "ppe_stream_session_dev.h"
#include "ppe_internal.h"

extern "C" uint32_t ppe_stream_session_step(uint32_t record[16], const uint32_t pkt[7], uint64_t *counters) {
    if (!record || !pkt) return 0u;
    PpeSsn x;
    ppe_ss_unpack(record, x);
    const PpeSsPkt p = {pkt[0] & 0xffu, pkt[1], pkt[2], pkt[3] & 0xffffu, pkt[4] & 0xffffu, pkt[5] & 0xffu, pkt[6] & 1u};
    const uint32_t r = ppe_stream_step(x, p, [&](uint32_t f) {
        if (counters) ++counters[f];
    });
    ppe_ss_pack(x, record);
    return r;
}
