// checkpoint_dump -- runs the layout and the checkpoint conversions of csrc/usim_checkpoint.h on host arrays read from a file, for tests/test_checkpoint_host.py.
// A host program: no HIP call, no GPU.
//   checkpoint_dump KIND N IN OUT            KIND: rigid | top | warm (top face with the warm rows) | full
// IN, raw little-endian, one behind the other:
//   block    float32 [nfields * npad]        a device block to write into (any bit patterns: what a conversion does not own must come through)
//   scalars  float32 [N][40]                 lattice  float32 [N][n_el][2] (none: rigid)
//   full:    base float32 [3], body float64 [N][USIM_FULL_BODY_WORDS]          warm:  w float32 [N][USIM_WARM_WORDS]
// Output: the fields of the layout, one "name value" line each, and the files OUT.<name>, raw:
//   state_dev   block after state_words<TO_DEVICE>(scalars, lattice)      state_scalars, state_lattice   state_words<TO_HOST> of state_dev
//   body_dev    the block's lattice region after body_words<TO_DEVICE>(body)     body_back  body_words<TO_HOST> of body_dev     body_dev2  the region after <TO_DEVICE>(body_back)
//   warm_empty  npad rows after empty_warm      warm_dev   warm_words<TO_DEVICE>(w)     warm_back  warm_words<TO_HOST> of warm_dev
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/usim.h"
#include "../robotic-ultrasound-imaging_amd/csrc/usim_device.h"
#include "../robotic-ultrasound-imaging_amd/csrc/usim_checkpoint.h"

using namespace usim;

template <class T> static std::vector<T> take(std::FILE* f, size_t count) {
    std::vector<T> v(count);
    if (count && std::fread(v.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "checkpoint_dump: the input is too short\n"); std::exit(1); }
    return v;
}
template <class T> static void put(const std::string& out, const char* name, const std::vector<T>& v) {
    std::FILE* f = std::fopen((out + "." + name).c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size() || std::fclose(f) != 0) { std::perror("checkpoint_dump: output"); std::exit(1); }
}

int main(int argc, char** argv) {
    const std::string kind = argc == 5 ? argv[1] : "";
    const bool rigid = kind == "rigid", top = kind == "top", warm = kind == "warm", full = kind == "full";
    if (!(rigid || top || warm || full) || std::atoi(argv[2]) <= 0) { std::fprintf(stderr, "usage: checkpoint_dump rigid|top|warm|full N IN OUT\n"); return 2; }
    const StateLayout L = state_layout(full ? USIM_TORSO_FULL : rigid ? USIM_TORSO_NONE : USIM_TORSO_TOP, full ? NSH : rigid ? 0 : N_TOP, std::atoi(argv[2]), warm);
    std::printf("n %d\nnpad %d\nn_el %d\nnfields %d\nlat_words %d\nlat_s %d\nlat_sd %d\nbank_row0 %d\nwarm_words %d\nwords %zu\nlive_words %zu\nlattice0 %zu\nwarm0 %zu\nsnapshot_words %d\n",
                L.n, L.npad, L.n_el, L.nfields, L.lat_words, L.lat_s, L.lat_sd, L.bank_row0, L.warm_words, L.words, L.live_words(), L.lattice(0), L.warm(0), L.snapshot_words());
    std::FILE* in = std::fopen(argv[3], "rb");
    if (!in) { std::perror("checkpoint_dump: input"); return 1; }
    const std::string out = argv[4];
    const std::vector<float> block = take<float>(in, L.live_words()), scalars = take<float>(in, (size_t)L.n * USIM_NSCALAR), lattice = take<float>(in, (size_t)L.n * L.n_el * 2);

    std::vector<float> dev = block, sc(scalars.size()), lat(lattice.size());
    state_words<TO_DEVICE>(L, dev.data(), scalars.data(), L.n_el ? lattice.data() : nullptr);
    state_words<TO_HOST>(L, dev.data(), sc.data(), L.n_el ? lat.data() : nullptr);
    put(out, "state_dev", dev); put(out, "state_scalars", sc); put(out, "state_lattice", lat);

    if (full) {
        const std::vector<float> base = take<float>(in, 3);
        const std::vector<double> body = take<double>(in, (size_t)L.n * USIM_FULL_BODY_WORDS);
        std::vector<float> region(block.begin() + L.lattice(0), block.end()), region2 = region;
        std::vector<double> back(body.size());
        body_words<TO_DEVICE>(L, base.data(), region.data(), body.data());
        body_words<TO_HOST>(L, base.data(), region.data(), back.data());
        body_words<TO_DEVICE>(L, base.data(), region2.data(), back.data());
        put(out, "body_dev", region); put(out, "body_back", back); put(out, "body_dev2", region2);
    }
    if (warm) {
        const std::vector<float> w = take<float>(in, (size_t)L.n * USIM_WARM_WORDS);
        std::vector<float> empty((size_t)L.npad * L.warm_words, 1.5f), rows(w.size()), back(w.size());
        empty_warm(L.npad, empty.data());
        warm_words<TO_DEVICE>(L.n, rows.data(), w.data());
        warm_words<TO_HOST>(L.n, rows.data(), back.data());
        put(out, "warm_empty", empty); put(out, "warm_dev", rows); put(out, "warm_back", back);
    }
    std::fclose(in);
    return 0;
}
