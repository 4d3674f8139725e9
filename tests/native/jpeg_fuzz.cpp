// Host-only driver for the sanitizer test of the JPEG coefficient decoder (csrc/jpeg.cpp):
// decodes every file named on the command line at its frame-header size and at a wrong
// size, from memory and from its path, into buffers of exactly the sizes the ABI states,
// so AddressSanitizer / UndefinedBehaviorSanitizer see every parser path on hostile
// input.  Every parameter record the decoder produces must pass mlg_jpeg_params_check
// against mlg_jpeg_coef_bytes.  Built and run by tests/test_jpeg_sanitizers.py; never part
// of the product.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/mlgate.h"

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> b;
    if (FILE* f = std::fopen(path, "rb")) {
        int c;
        while ((c = std::fgetc(f)) != EOF) b.push_back((uint8_t)c);
        std::fclose(f);
    }
    return b;
}

int main(int argc, char** argv) {
    int ok = 0, bad = 0;
    for (int i = 1; i < argc; ++i) {
        std::vector<uint8_t> b = slurp(argv[i]);
        const uint8_t* p = b.empty() ? nullptr : b.data();
        int32_t info[8] = {0};
        int w = 16, h = 16;
        if (p && mlg_jpeg_info(p, b.size(), info) == MLG_OK && info[0] > 0 && info[1] > 0 &&
            (long)info[0] * info[1] <= (1L << 20)) {
            w = info[0];
            h = info[1];
        }
        for (int pass = 0; pass < 3; ++pass) {
            const int H = pass == 1 ? h + 1 : h, W = w;
            const size_t bytes = mlg_jpeg_coef_bytes(H, W);
            if (bytes == 0 || bytes % 128) return 5;
            std::vector<int16_t> coefs(bytes / 2);
            std::vector<uint16_t> qtabs(192);
            std::vector<int32_t> params(MLG_JPEG_PARAMS, -1);
            int32_t st = 0;
            if (pass < 2) {
                const uint8_t* ptrs[1] = {p ? p : (const uint8_t*)""};
                const size_t lens[1] = {b.size()};
                if (mlg_jpeg_coefs_decode(ptrs, lens, 1, coefs.data(), qtabs.data(), params.data(), H, W, 1, &st) != MLG_OK)
                    return 2;
            } else {
                const char* paths[1] = {argv[i]};
                if (mlg_jpeg_coefs_load(paths, 1, coefs.data(), qtabs.data(), params.data(), H, W, 2, &st) != MLG_OK)
                    return 3;
            }
            // a produced record must fit the buffer; a failed image must leave an empty one
            if (mlg_jpeg_params_check(params.data(), 1, H, W, bytes) != MLG_OK) return 4;
            if ((st == MLG_OK) != (params[0] != 0)) return 6;
            if (pass < 2) (st == MLG_OK ? ok : bad) += 1;
        }
    }
    std::printf("decoded %d, rejected %d\n", ok, bad);
    return 0;
}
