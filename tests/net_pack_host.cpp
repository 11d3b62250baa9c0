// net_pack_host.cpp — runs every packer of tak_amd/csrc/net_pack.h on the CPU (tests/test_net_pack.py builds it with the host
// compiler, plain and under the address / undefined-behaviour sanitizers) and writes each result as a raw array into argv[1].
// Inputs: tensor `salt`, element i = pat(i, salt), a fixed integer pattern the test restates in numpy.
#include <cstdio>
#include <cstdlib>

#include "net_pack.h"

using namespace tg;

static std::string dir;

// a multiple of 1/256 in [-128, 128): 16 significant bits, so the bf16 split has a low half that is not zero
static float pat(size_t i, unsigned salt) {
    uint32_t h = (uint32_t)i * 2654435761u + salt * 40503u;
    return (float)((int)((h >> 8) & 0xffffu) - 32768) / 256.0f;
}
static std::vector<float> tensor(size_t count, unsigned salt) {
    std::vector<float> v(count);
    for (size_t i = 0; i < count; i++) v[i] = pat(i, salt);
    return v;
}
template <class T>
static void dump(const std::string& name, const std::vector<T>& v) {
    FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size() || std::fclose(f) != 0) {
        std::fprintf(stderr, "cannot write %s\n", name.c_str());
        std::exit(2);
    }
}
static Folded folded(int O, int I, unsigned salt) { return Folded{tensor((size_t)O * I * 9, salt), tensor(O, salt + 1)}; }

// the three FC layouts of one shape; the value column where the padding leaves room, as net_finalize decides it
static void fc_f32(const std::string& tag, int F, int nsq, int P, unsigned salt) {
    const size_t K = (size_t)F * nsq;
    const int NP = fc_padded_cols(K, P);
    auto w = tensor(P * K, salt), b = tensor(P, salt + 1), wv = tensor(K, salt + 2);
    FcColumns c{w.data(), b.data(), NP > P ? wv.data() : nullptr, pat(0, salt + 3), P, F, nsq};
    auto wp = pack_fc(c, NP);
    dump(tag + "_w", wp);
    dump(tag + "_lanes", pack_fc_lanes(wp, NP));
    dump(tag + "_b", c.bias(NP));
    dump(tag + "_np", std::vector<int32_t>{NP, c.cols()});
}
static void fc_split(const std::string& tag, int F, int nsq, int P, int CB, int ring_tiles, unsigned salt) {
    const size_t K = (size_t)F * nsq;
    const int NP = round_up(P, CB);
    auto w = tensor(P * K, salt), b = tensor(P, salt + 1), wv = tensor(K, salt + 2);
    FcColumns c{w.data(), b.data(), NP > P ? wv.data() : nullptr, pat(0, salt + 3), P, F, nsq};
    dump(tag + "_w", pack_fc_s3(c, NP, CB));
    dump(tag + "_b", c.bias(NP));
    if (ring_tiles) dump(tag + "_ring", pack_fc_s3_ring(c, ring_tiles));
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    dir = argv[1];
    {   // find, fold_conv_bn: O = 5, I = 26; the variance tensor made positive
        const int O = 5, I = 26;
        TensorMap t;
        t["c.weight"] = tensor((size_t)O * I * 9, 1);
        t["c.bias"] = tensor(O, 2);
        t["n.weight"] = tensor(O, 3);
        t["n.bias"] = tensor(O, 4);
        t["n.running_mean"] = tensor(O, 5);
        t["n.running_var"] = tensor(O, 6);
        for (auto& v : t["n.running_var"]) v = std::fabs(v) + 0.5f;
        Folded f, raw;
        std::string err, log;
        if (!fold_conv_bn(t, "c", "n", O, I, f, err) || !fold_conv_bn(t, "c", "", O, I, raw, err)) return 3;
        dump("fold_w", f.w);
        dump("fold_b", f.b);
        dump("fold_raw_w", raw.w);
        // the messages of a missing and of a mis-sized tensor, in the order of discovery
        t.erase("n.running_mean");
        t["n.bias"].push_back(0.0f);
        log += fold_conv_bn(t, "c", "n", O, I, f, err) ? "ok\n" : err + "\n";
        t["n.bias"].pop_back();
        log += fold_conv_bn(t, "c", "n", O, I, f, err) ? "ok\n" : err + "\n";
        log += fold_conv_bn(t, "d", "n", O, I, f, err) ? "ok\n" : err + "\n";
        dump("errors.txt", std::vector<char>(log.begin(), log.end()));
    }
    {   // f32 conv layout: a partly filled last chunk (26 of 32 channels), OP padding (5 → 64), the last chunk in order and permuted
        const Folded f = folded(5, 26, 10);
        std::vector<float> w, b;
        pack_conv(f, 5, 26, 32, 4, w, b);
        dump("conv_t4_w", w);
        dump("conv_t4_b", b);
        pack_conv(f, 5, 26, 32, 3, w, b);
        dump("conv_t3_w", w);
        dump("conv_t3_b", b);
    }
    // split conv fragments: two waves' worth of the tile / row interleave with a ragged channel chunk, and the head's 36 → 64
    dump("conv_s3_64", pack_conv_s3(folded(64, 40, 20), 64, 40, 2));
    dump("conv_s3_36", pack_conv_s3(folded(36, 40, 22), 36, 40, 2, 64));
    {   // board restriction and S: O = 3, I = 7, the first 2 planes are board planes
        const Folded f = folded(3, 7, 30);
        const Folded fb = restrict_to_board(f, 3, 7, 2);
        dump("board_w", fb.w);
        dump("board_b", fb.b);
        dump("cplane_sums", pack_cplane_sums(f, 3, 7, 2));
    }
    fc_f32("fc_k64_p30", 16, 4, 30, 40);   // K % 64 == 0: NP = 208, value column at 30
    fc_f32("fc_k72_p30", 8, 9, 30, 44);    // K = 72: NP = round_up(P, 64) = 64, value column at 30
    fc_f32("fc_k72_p64", 8, 9, 64, 48);    // NP = P: no value column
    fc_split("s3_p100", 16, 4, 100, 112, 8, 52);  // NP = 112, value column at 100; the ring layout with 8 tiles
    fc_split("s3_p112", 16, 4, 112, 112, 0, 56);  // no room for the value column
    {
        auto wv = tensor(64, 60);
        dump("value_w", pack_value(wv.data(), 16, 4));
    }
    {   // bf16 rounding and split on values that tie, carry, overflow to infinity, and on the non-finite ones
        const uint32_t bits[] = {0x00000000u, 0x80000000u, 0x3f808000u, 0x3f818000u, 0x3f807fffu, 0x3f808001u, 0x3fffffffu, 0x7f7fffffu,
                                 0x7f800000u, 0xff800000u, 0x7fc00001u, 0x00000001u, 0x00ffffffu, 0xc0490fdbu, 0x3dcccccdu, 0x477fe000u};
        std::vector<float> x;
        std::vector<uint16_t> hi, lo;
        for (uint32_t u : bits) {
            float v;
            std::memcpy(&v, &u, 4);
            x.push_back(v);
        }
        for (size_t i = 0; i < 64; i++) x.push_back(pat(i, 70) * 0.37f);
        for (float v : x) {
            uint16_t h, l;
            split_bf16(v, h, l);
            hi.push_back(h);
            lo.push_back(l);
            if (h != f32_to_bf16(v)) return 4;
        }
        dump("bf16_x", x);
        dump("bf16_hi", hi);
        dump("bf16_lo", lo);
    }
    {   // round_up and the FC padding rule
        std::vector<int32_t> r;
        for (int K : {64, 72, 1600, 2400})
            for (int P : {1, 30, 64, 208, 209, 1575}) r.push_back(fc_padded_cols((size_t)K, P));
        for (int v : {0, 1, 63, 64, 65, 1575}) r.push_back(round_up(v, 112));
        dump("padding", r);
    }
    return 0;
}
