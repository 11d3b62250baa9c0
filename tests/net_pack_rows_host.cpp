// net_pack_rows_host.cpp — runs pack_board_rows of tak_amd/csrc/net_pack.h on the CPU (tests/test_net_pack_rows.py builds it with the
// host compiler, plain and under the address / undefined-behaviour sanitizers) and writes the result as a raw array into argv[1].
// Input: a folded conv0 whose element i is pat(i, salt), the integer pattern of tests/net_pack_host.cpp.
#include <cstdio>
#include <cstdlib>

#include "net_pack.h"

using namespace tg;

static float pat(size_t i, unsigned salt) {
    uint32_t h = (uint32_t)i * 2654435761u + salt * 40503u;
    return (float)((int)((h >> 8) & 0xffffu) - 32768) / 256.0f;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const int O = 6, I = 11, bc = 4;  // 4 board planes of 11 input planes, 6 output channels
    Folded f;
    f.w.resize((size_t)O * I * 9);
    f.b.resize(O);
    for (size_t i = 0; i < f.w.size(); i++) f.w[i] = pat(i, 80);
    for (size_t i = 0; i < f.b.size(); i++) f.b[i] = pat(i, 81);
    const std::vector<float> R = pack_board_rows(f, O, I, bc);
    FILE* out = std::fopen((std::string(argv[1]) + "/board_rows").c_str(), "wb");
    if (!out || std::fwrite(R.data(), sizeof(float), R.size(), out) != R.size() || std::fclose(out) != 0) return 3;
    return 0;
}
