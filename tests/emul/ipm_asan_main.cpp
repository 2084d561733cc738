// ipm_asan_main.cpp — the interior-point entries of tests/prims/ipm_entries.h as a stand-alone program for the
// AddressSanitizer + UBSan run of the CPU tier (TEST INFRASTRUCTURE ONLY; tests/emul_ipm_asan.py builds and runs it).
//
//   ipm_asan_main IN OUT
// IN : int64 kind, B, blob bytes, n_out, seed; per case 31 int64 (d, p, nnz, nlong, nteam, mode, flags, n_seq, ldh, empty,
//      n_outf, n_out, n_in[4], the byte offsets into the blob of mptr, mcol, mval, cptr, cvar, cvalc, usign, vkind,
//      longrow, teamrow, fin, in[4]) and the element offset of its outputs; then the blob (emul_lib.op_pack).
// OUT: int32 rc; out [n_out] doubles; outi [4 B] int32.
// The blob, the outputs and the workgroup's LDS (simt_abi.cpp Lds) are heap blocks of their exact sizes: a read or write
// past any of them stops the program.  Prints "ipm-asan-ok".
#define CAVE_SIMT_OPS
#include "simt_abi.cpp"

#include <cstdio>

namespace {

template <class T>
std::vector<T> read_n(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}
template <class T>
void write_n(FILE* f, const std::vector<T>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short output\n"); exit(2); }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  const std::vector<int64_t> hd = read_n<int64_t>(in, 5);
  const int32_t kind = (int32_t)hd[0];
  const int64_t B = hd[1], nblob = hd[2], n_out = hd[3];
  if (B < 0 || B > 256 || nblob < 0 || n_out < 0) return 3;
  const std::vector<int64_t> rec = read_n<int64_t>(in, (size_t)B * 32);
  const std::vector<unsigned char> blob = read_n<unsigned char>(in, (size_t)nblob);
  fclose(in);
  std::vector<double> out((size_t)n_out, cave_prims::poison_f64());
  std::vector<int32_t> outi((size_t)B * 4, -7);
  std::vector<cave_ops::OpCase> cases((size_t)B);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t* r = rec.data() + b * 32;
    cave_ops::OpCase& k = cases[(size_t)b];
    k = cave_ops::OpCase{};
    k.d = (int32_t)r[0]; k.p = (int32_t)r[1]; k.nnz = (int32_t)r[2]; k.nlong = (int32_t)r[3]; k.nteam = (int32_t)r[4];
    k.mode = (int32_t)r[5]; k.flags = (int32_t)r[6]; k.n_seq = (int32_t)r[7]; k.ldh = (int32_t)r[8]; k.empty = (int32_t)r[9];
    k.n_outf = (int32_t)r[10]; k.n_out = (int32_t)r[11];
    for (int i = 0; i < 4; ++i) k.n_in[i] = (int32_t)r[12 + i];
    const unsigned char* base = blob.data();
    k.mptr = reinterpret_cast<const uint32_t*>(base + r[16]);
    k.mcol = reinterpret_cast<const uint16_t*>(base + r[17]);
    k.mval = reinterpret_cast<const float*>(base + r[18]);
    k.cptr = reinterpret_cast<const uint32_t*>(base + r[19]);
    k.cvar = reinterpret_cast<const uint16_t*>(base + r[20]);
    k.cvalc = reinterpret_cast<const float*>(base + r[21]);
    k.usign = base + r[22];
    k.vkind = base + r[23];
    k.longrow = reinterpret_cast<const uint32_t*>(base + r[24]);
    k.teamrow = reinterpret_cast<const uint32_t*>(base + r[25]);
    k.fin = reinterpret_cast<const float*>(base + r[26]);
    for (int i = 0; i < 4; ++i) k.in[i] = reinterpret_cast<const double*>(base + r[27 + i]);
    if (r[31] < 0 || r[31] + k.n_out > n_out) return 3;
    k.out = out.data() + r[31];
    k.outf = nullptr;
    k.outi = outi.data() + 4 * b;
  }
  const int32_t rc = cave_simt_op_run(kind, cases.data(), B, (uint64_t)hd[4]);
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  write_n(fo, std::vector<int32_t>{rc});
  write_n(fo, out);
  write_n(fo, outi);
  fclose(fo);
  printf("ipm-asan-ok\n");
  return 0;
}
