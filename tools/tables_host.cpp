// tables_host.cpp — the host work of mnx_set_vocab_text, mnx_set_symbol_tables and mnx_set_fragments
// (molnextr_amd/csrc/table_host.h: the caller's offsets and records validated, the image the device reads laid out) as a program
// on the host, so that the host compiler's sanitizers see the very text the library runs:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/tables_host.cpp -o tables_host
// Every array a case hands to a builder is a heap block of exactly the elements the case lists, so a read behind one is a report.
// stdin: the number of cases; then per case, whitespace between all items, a list being its length and then its items, bytes being
// a list of numbers, `null` a bit mask of the arguments passed as null pointers in the order of the signature:
//   V sym_offset n null offsets[] bytes[]
//   S n null offsets[] kinds[] bytes[]
//   F n_frags na nb nt n_names st_n null mols[][atom0 n_atoms bond0 n_bonds text0 smiles_len] atoms[][sym0 sym_len]
//     bonds[][i j type rev] text[] frag_of_name[] st_kind[]
// stdout, per case: `refused <message>`, or `ok` (F: `ok off0 off1 off2 off3 off4`) and a line with the image in hex. Exit status 2
// and a message on stderr for input that is no such description.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../molnextr_amd/csrc/table_host.h"

static long long number() {
    long long v;
    if (std::scanf("%lld", &v) != 1) {
        std::fprintf(stderr, "tables_host: a number is missing\n");
        std::exit(2);
    }
    return v;
}

template <typename T>
static std::vector<T> list() {
    const long long n = number();
    if (n < 0 || n > (1 << 20)) {
        std::fprintf(stderr, "tables_host: no list of %lld items\n", n);
        std::exit(2);
    }
    std::vector<T> v((size_t)n);
    for (T& x : v) x = (T)number();
    return v;
}

// the pointer a builder receives for a list: null where the case says so (an empty list keeps its one-past-the-end pointer)
template <typename T>
static const T* arg(const std::vector<T>& v, long long null, int bit) {
    return null >> bit & 1 ? nullptr : v.data();
}

static void print_image(const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) std::printf("%02x", ((const unsigned char*)p)[i]);
    std::printf("\n");
}

int main() {
    const long long cases = number();
    for (long long c = 0; c < cases; ++c) {
        char kind = 0;
        if (std::scanf(" %c", &kind) != 1) kind = 0;
        if (kind == 'V') {
            const int sym_offset = (int)number(), n = (int)number();
            const long long null = number();
            const std::vector<uint32_t> offsets = list<uint32_t>();
            const std::vector<char> bytes = list<char>();
            mnx::VocabText vt;
            const std::string why = mnx::build_vocab_text(arg(bytes, null, 0), arg(offsets, null, 1), n, sym_offset, &vt);
            if (!why.empty()) { std::printf("refused %s\n", why.c_str()); continue; }
            std::printf("ok\n");
            print_image(&vt, sizeof(vt));
        } else if (kind == 'S') {
            const int n = (int)number();
            const long long null = number();
            const std::vector<uint32_t> offsets = list<uint32_t>();
            const std::vector<uint8_t> kinds = list<uint8_t>();
            const std::vector<char> bytes = list<char>();
            auto st = std::make_unique<mnx::SymbolTables>();
            const std::string why = mnx::build_symbol_tables(arg(bytes, null, 0), arg(offsets, null, 1), arg(kinds, null, 2), n, st.get());
            if (!why.empty()) { std::printf("refused %s\n", why.c_str()); continue; }
            std::printf("ok\n");
            print_image(st.get(), sizeof(mnx::SymbolTables));
        } else if (kind == 'F') {
            const int n_frags = (int)number();
            const uint32_t na = (uint32_t)number(), nb = (uint32_t)number(), nt = (uint32_t)number();
            const int n_names = (int)number(), st_n = (int)number();
            const long long null = number();
            std::vector<mnx_mol> mols((size_t)number());
            for (mnx_mol& m : mols) {
                m = mnx_mol{};
                m.atom0 = (uint32_t)number(); m.n_atoms = (uint32_t)number(); m.bond0 = (uint32_t)number();
                m.n_bonds = (uint32_t)number(); m.text0 = (uint32_t)number(); m.smiles_len = (uint32_t)number();
            }
            std::vector<mnx_atom> atoms((size_t)number());
            for (mnx_atom& a : atoms) {
                a = mnx_atom{};
                a.sym0 = (uint32_t)number(); a.sym_len = (uint16_t)number();
            }
            std::vector<mnx_bond> bonds((size_t)number());
            for (mnx_bond& b : bonds) {
                b = mnx_bond{};
                b.i = (uint16_t)number(); b.j = (uint16_t)number(); b.type = (uint8_t)number(); b.rev = (uint8_t)number();
            }
            const std::vector<char> text = list<char>();
            const std::vector<int32_t> frag_of_name = list<int32_t>();
            const std::vector<unsigned char> st_kind = list<unsigned char>();
            if ((long long)st_kind.size() < st_n) {
                std::fprintf(stderr, "tables_host: fewer kinds than st_n (case %lld)\n", c);
                return 2;
            }
            mnx::FragImage img;
            const std::string why = mnx::build_fragments(arg(mols, null, 0), n_frags, arg(atoms, null, 1), na, arg(bonds, null, 2), nb,
                                                         arg(text, null, 3), nt, arg(frag_of_name, null, 4), n_names, st_kind.data(), st_n, &img);
            if (!why.empty()) { std::printf("refused %s\n", why.c_str()); continue; }
            std::printf("ok %zu %zu %zu %zu %zu\n", img.off[0], img.off[1], img.off[2], img.off[3], img.off[4]);
            print_image(img.blob.data(), img.blob.size());
        } else {
            std::fprintf(stderr, "tables_host: case %lld is no V, S or F\n", c);
            return 2;
        }
    }
    return 0;
}
