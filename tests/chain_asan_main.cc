// tests/chain_asan_main.cc — hevc_amd/csrc/chain_plan.h alone under the sanitizers (test_chain_cpu.py builds this with -fsanitize=address,undefined): every slot
// combination over good and bad sizes, depths, selectors, strengths and reserved words, frame counts up to 2^40.  Host code only; no device, no python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>

#include "../hevc_amd/csrc/chain_plan.h"

using namespace mihevc;

static int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); fails++; } \
    } while (0)

int main()
{
    long tried = 0, valid = 0;
    const int sizes[][2] = {{52, 36}, {100, 68}, {200, 136}, {50, 34}, {16, 16}, {14, 36}, {53, 36}, {8192, 8192}, {8194, 64}, {-4, 36}, {0x7ffffffe, 0x7ffffffc}};
    const int64_t counts[] = {0, 1, 2, 5, 6, 12, (int64_t)1 << 40};
    CHECK(!chain_check(nullptr, 100, 68, 8, 1, 0));
    for (int field = -1; field <= 3; field++)
        for (int fsub = 0; fsub < 4; fsub++)
            for (int dn = -1; dn <= 2; dn++)
                for (int resize = -1; resize <= 4; resize++)
                    for (int factor = 0; factor <= 5; factor++)
                        for (auto &sz : sizes)
                            for (int depth : {8, 10, 12})
                                for (int sr_scale : {0, 2, 3, 4}) {
                                    // the descriptor lives in a block of exactly its size: a read past it is the sanitizer's to report
                                    std::unique_ptr<unsigned char[]> block(new unsigned char[sizeof(mihevc_chain)]);
                                    mihevc_chain *c = new (block.get()) mihevc_chain();
                                    c->width = sz[0]; c->height = sz[1]; c->bit_depth = depth;
                                    c->field = field; c->denoise_on = dn == 2 ? 1 : dn; c->resize = resize; c->interpolate_on = factor != 0;
                                    c->deint.tff = fsub & 1; c->deint.field_rate = fsub >> 1;
                                    c->fieldmatch.tff = 1; c->fieldmatch.decimate = fsub & 1; c->fieldmatch.deint = fsub >> 1;
                                    c->denoise.luma_spatial = 5; c->denoise.luma_temporal = 7; c->denoise.chroma_spatial = 5; c->denoise.chroma_temporal = dn == 2 ? 256 : 7;
                                    c->upscale.width = sz[0]; c->upscale.height = sz[1]; c->upscale.bit_depth = depth; c->upscale.sharpen = 8; c->upscale.antiring = 8;
                                    c->sr.width = sz[0]; c->sr.height = sz[1]; c->sr.bit_depth = depth; c->sr.matrix = 6; c->sr.full_range = 0;
                                    c->interpolate.factor = factor; c->interpolate.mode = 0; c->interpolate.scene_threshold = 10;
                                    tried++;
                                    const int W = 100, H = 68, D = 8;
                                    if (!chain_check(c, W, H, D, 1, sr_scale)) continue;
                                    valid++;
                                    const ChainPlan p = chain_plan(*c, W, H, D);
                                    CHECK(p.stages >= 1 && p.stages <= 4 && p.rate_num >= 1 && p.rate_den >= 1 && chain_gcd(p.rate_num, p.rate_den) == 1);
                                    CHECK(p.sw == sz[0] && p.sh == sz[1] && p.dw == W && p.dh == H);
                                    CHECK(p.resize || (p.sw == W && p.sh == H && p.sd == D));
                                    const bool bob = field == MIHEVC_CHAIN_FIELD_DEINT && (fsub >> 1), dec = field == MIHEVC_CHAIN_FIELD_MATCH && (fsub & 1);
                                    int64_t last = -1;
                                    for (int64_t n : counts) {
                                        const int64_t got = chain_pictures(*c, n);
                                        int64_t want = n;
                                        if (bob) want *= 2;
                                        if (dec) want -= want / 5;
                                        if (factor && want > 0) want = factor * (want - 1) + 1;
                                        CHECK(got == want && got >= last);
                                        last = got;
                                    }
                                    // ten frames are two whole cycles: the count is the rate's, but for the interpolator's missing last pictures
                                    const int64_t base = 10 * (bob ? 2 : 1) * (dec ? 4 : 5) / 5;
                                    CHECK(base * (factor ? factor : 1) * p.rate_den == 10 * (int64_t)p.rate_num);
                                    // a set reserved word, anywhere it is looked at, is refused
                                    c->reserved[8] = 1;
                                    CHECK(!chain_check(c, W, H, D, 1, sr_scale));
                                    c->reserved[8] = 0;
                                    // and so is a session whose size or depth no chain takes
                                    CHECK(!chain_check(c, 101, H, D, 1, sr_scale) && !chain_check(c, W, H, 9, 1, sr_scale) && !chain_check(c, W, 14, D, 1, sr_scale));
                                }
    if (fails) return 1;
    std::printf("%ld descriptors, %ld valid\n", tried, valid);
    return 0;
}
