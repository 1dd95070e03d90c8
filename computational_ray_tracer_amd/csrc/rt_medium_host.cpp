// rt_medium_transmittance (include/rtmi355x.h): rt_medium.h's transmittance on the host, no context and
// no HIP runtime.  A file of its own so that a plain host compiler builds it: tests/test_medium_reference.py compiles it
// with a stand-alone main under -fsanitize=address,undefined.
#include <cstddef>
#include <string>

#include "rt_guard.h"
#include "rt_medium.h"
#include "../../include/rtmi355x.h"

extern "C" int rt_medium_transmittance(const rt_medium* m, int n, const float* lambda, const float* len, float* out) {
    return rtmi::guarded([&] {
        if (n < 0 || (n && (!m || !lambda || !len || !out))) return (int)RT_E_ARG;
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < 8; ++k)
                out[8 * (size_t)i + k] = rtmi::medium_transmittance(m[i].sigmoid[0], m[i].sigmoid[1], m[i].sigmoid[2],
                                                                    m[i].sigma, lambda[8 * (size_t)i + k], len[i]);
        return (int)RT_OK;
    }, [](const std::string&) {});
}
