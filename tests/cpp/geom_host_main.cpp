// geom_host_main.cpp -- the kernel geometry of an encoder context
// (zig-flac_amd/csrc/fg_geom.hpp: enc_geometry) on the host.  A stand-alone program, built by
// tests/test_geom_host.py with -fsanitize=address,undefined (and once more with -DFG_DIAG=1 for the
// diagnostic knobs): which kernel variant, thread count and LDS size a configuration gets, and
// whether it is refused, without a device.
//
//   geom_host_main CHANNELS BITS PREDICTION STEREO_DECORRELATION BLOCK_SIZE [FLACGPU_KNOB=TEXT ...]
//
// The knobs are given as the library would find them in its environment.  Prints the EncGeom as one
// JSON object, {"rc": 0, "C": ..., ...}, or {"rc": -1} for a refused configuration.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

// host only: fg_layout.hpp's functions are plain inline functions here
#define __host__
#define __device__
#include "../../zig-flac_amd/csrc/fg_geom.hpp"

int main(int argc, char **argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: geom_host_main CHANNELS BITS PREDICTION STEREO BLOCK [FLACGPU_KNOB=TEXT ...]\n");
        return 2;
    }
    flacgpu_config cfg{};
    cfg.sample_rate = 44100;
    cfg.channels = (uint8_t)std::atoi(argv[1]);
    cfg.bits_per_sample = (uint8_t)std::atoi(argv[2]);
    cfg.prediction = (uint8_t)std::atoi(argv[3]);
    cfg.stereo_decorrelation = (uint8_t)std::atoi(argv[4]);
    cfg.block_size = (uint16_t)std::atoi(argv[5]);
    cfg.max_rice_part_order = 8;
    cfg.max_rice_param = 30;
    fg::Knobs k;
    for (int i = 6; i < argc; i++) {
        const char *eq = std::strchr(argv[i], '=');
        if (!eq || !fg::knob_set(k, std::string(argv[i], (size_t)(eq - argv[i])).c_str(), eq + 1)) {
            std::fprintf(stderr, "not a knob of this build: %s\n", argv[i]);
            return 2;
        }
    }
    fg::EncGeom g;
    const int rc = fg::enc_geometry(cfg, k, g);
    if (rc) {
        std::printf("{\"rc\": %d}\n", rc);
        return 0;
    }
    std::printf("{\"rc\": 0");
#define U(f) std::printf(", \"" #f "\": %u", (unsigned)g.f)
    U(C); U(B); U(bits); U(stereo);
    U(nt); U(nt_pack); U(nt_pack4); U(nt_split); U(nt_psplit);
    U(lds); U(lds_tail); U(lds_pack); U(lds_pack4); U(lds_split); U(lds_psplit);
    U(image_bytes); U(image_split); U(desc_stride);
    U(crc_hmax); U(crc_hmax4); U(crc_hmaxs);
    U(stage_dbuf); U(pack_dbuf); U(ana_split); U(pack_split);
    std::printf(", \"md5_kernel\": %d", g.md5_kernel);
    U(ana1); U(ana1_variant); U(fused); U(lds_fused); U(crc_hmaxf);
#undef U
    std::printf("}\n");
    return 0;
}
