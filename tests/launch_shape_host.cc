// Host-only check of the launch arithmetic (supernova_amd/csrc/snk_launch.h without HIP): built and run by
// tests/test_abi.py::test_launch_arithmetic_on_the_host.  Every value follows from the header's definitions; none is a measurement.
#include <stdio.h>

#include "snk_launch.h"

static int failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED: %s\n", #cond); failed = 1; } } while (0)

int main() {
    const uint64_t one = 1;
    CHECK(snk_blocks(0, 256) == 0);
    CHECK(snk_blocks(1, 256) == 1);
    CHECK(snk_blocks(256, 256) == 1);
    CHECK(snk_blocks(257, 256) == 2);
    CHECK(snk_blocks(one << 40, 256) == one << 32);             // no truncation to 32 bits
    CHECK(snk_blocks(~(uint64_t)0, 256) == one << 56);          // ... and no wrap in the rounding
    CHECK(snk_blocks_capped(0, 256, one << 20) == 1);
    CHECK(snk_blocks_capped(one << 40, 256, one << 20) == one << 20);
    CHECK(snk_blocks_capped(one << 40, 256, 65536) == 65536);
    CHECK(snk_blocks_capped(1000, 256, 65536) == 4);
    CHECK(snk_launch_shape_ok((one << 24) - 1, 256));
    CHECK(snk_launch_shape_ok(0, 256));
    CHECK(!snk_launch_shape_ok(one << 24, 256));                // 2^32 work items: refused (>=, not >)
    CHECK(!snk_launch_shape_ok(one << 31, 1));                  // more than 2^31 - 1 workgroups
    CHECK(snk_launch_shape_ok((one << 31) - 1, 1));
    CHECK(!snk_launch_shape_ok((one << 32) + 5, 64));           // a grid that a 32-bit cast would have turned into 5
    CHECK(!snk_launch_shape_ok(17400000, 256));                 // 4.45 G work items: the fragment copy that lost 87 % of the bases
    if (!failed) printf("ok\n");
    return failed;
}
