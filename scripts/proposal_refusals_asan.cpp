// The host-side argument checks of nerfhip_proposal_loss under AddressSanitizer and UBSan, on the CPU: a stand-alone program that makes
// the REFUSED calls only (and n == 0), so nothing is ever launched and no GPU is needed.  Build and run from the repository root:
//     hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Iinclude \
//         nerf-pytorch_amd/csrc/reg/proposal.hip nerf-pytorch_amd/csrc/elementwise.hip scripts/proposal_refusals_asan.cpp -o /tmp/refusals_asan
//     /tmp/refusals_asan
// Every refusal must return NERFHIP_ERR_ARG with its message and leave both outputs untouched; the exit status counts the misses.
#include <cstdio>
#include <cstring>
#include <vector>
#include "nerfhip.h"
int main() {
    std::vector<float> raw_c(4 * 5 * 4, 0.5f), z_c(4 * 5, 3.0f), raw_f(4 * 7 * 4, 0.5f), z_f(4 * 7, 3.0f), rays(4 * 8, 1.0f), loss(4, -7.0f), g(4 * 5, -7.0f);
    int bad = 0;
    auto refused = [&](const char* what, int rc, const char* match) {
        const char* msg = nerfhip_last_error();
        bool ok = rc == -1 && msg && strstr(msg, match);
        for (float v : loss) ok = ok && v == -7.0f;
        for (float v : g) ok = ok && v == -7.0f;
        printf("%-24s rc=%d %s [%s]\n", what, rc, ok ? "ok" : "BAD", msg ? msg : "");
        bad += !ok;
    };
#define CALL(rc_, zc, sc, rf, zf, sf, ry, stride, n, lo, gw) \
    nerfhip_proposal_loss(rc_, zc, sc, rf, zf, sf, ry, stride, n, 0.0f, nullptr, nullptr, 0, 0, 1.0f, nullptr, lo, gw, 0, nullptr)
    float *RC = raw_c.data(), *ZC = z_c.data(), *RF = raw_f.data(), *ZF = z_f.data(), *RY = rays.data(), *LO = loss.data(), *GW = g.data();
    refused("raw_coarse NULL", CALL(nullptr, ZC, 5, RF, ZF, 7, RY, 8, 4, LO, GW), "NULL");
    refused("z_coarse NULL", CALL(RC, nullptr, 5, RF, ZF, 7, RY, 8, 4, LO, GW), "NULL");
    refused("raw_fine NULL", CALL(RC, ZC, 5, nullptr, ZF, 7, RY, 8, 4, LO, GW), "NULL");
    refused("z_fine NULL", CALL(RC, ZC, 5, RF, nullptr, 7, RY, 8, 4, LO, GW), "NULL");
    refused("rays NULL", CALL(RC, ZC, 5, RF, ZF, 7, nullptr, 8, 4, LO, GW), "NULL");
    refused("ray_stride 7", CALL(RC, ZC, 5, RF, ZF, 7, RY, 7, 4, LO, GW), "ray_stride");
    refused("s_coarse 0", CALL(RC, ZC, 0, RF, ZF, 7, RY, 8, 4, LO, GW), "at least 1 sample");
    refused("s_fine -3", CALL(RC, ZC, 5, RF, ZF, -3, RY, 8, 4, LO, GW), "at least 1 sample");
    refused("cap + 1", CALL(RC, ZC, 4090, RF, ZF, 7, RY, 8, 4, LO, GW), "at most 4096");
    refused("INT_MAX-ish sum", CALL(RC, ZC, 2147483644, RF, ZF, 8, RY, 8, 4, LO, GW), "at most 4096");
    refused("both INT_MAX", CALL(RC, ZC, 2147483647, RF, ZF, 2147483647, RY, 8, 4, LO, GW), "at most 4096");
    refused("n < 0", CALL(RC, ZC, 5, RF, ZF, 7, RY, 8, -1, LO, GW), "n < 0");
    refused("both outputs NULL", CALL(RC, ZC, 5, RF, ZF, 7, RY, 8, 4, nullptr, nullptr), "both outputs");
    int rc = CALL(nullptr, nullptr, 5, nullptr, nullptr, 7, nullptr, 8, 0, nullptr, nullptr);
    printf("n == 0 rc=%d\n", rc);
    bad += rc != 0;
    printf(bad ? "FAILED %d\n" : "all refusals ok\n", bad);
    return bad;
}
