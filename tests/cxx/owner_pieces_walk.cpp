// The owner stiffness kernel's 16-byte pieces of a staged x plane (wave_fenics_amd/csrc/owner_pieces.h), walked on the
// host exactly as the kernel uses them: thread q % 256 owns piece q of every plane of its column; an inside piece is one
// 16-byte load from (plane base + off), a straddling piece one 8-byte load, an outside piece no load.
//
// For every mesh, P4 cross-section, column, plane of the first and of the last layer and both alignments of x
// (16-byte aligned, and 8 bytes past that) it checks that
//   * every load lies inside [x, x + ndofs) - by its byte range, and by doing it (memcpy) from a heap block of exactly
//     that size, which AddressSanitizer watches;
//   * every rectangle position inside the mesh is filled exactly once, with the x value of that lattice point;
//   * no position outside the mesh is ever loaded;
//   * a straddling piece has its first position in the mesh (the partner that is zeroed is the second), and a column has
//     at most RY of them.
// Prints "<n> failures".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "owner_pieces.h"

namespace {

long failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (++failures <= 20) {                             \
        std::printf("FAILED %s: ", #cond);                \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                                \
      }                                                   \
    }                                                     \
  } while (0)

double value_of(long dof) { return 1.0 + (double)dof; }   // distinct, never 0

struct Stats {
  long inside = 0, straddling = 0, outside = 0, columns = 0;
};

void walk(int nx, int ny, int BX, int BY, int shift, Stats& st)
{
  constexpr int P = 4, nz = 2;
  const wf::OwnerRect R = wf::owner_rect(P, BX, BY);
  const int NX = P * nx + 1, NY = P * ny + 1, NZ = P * nz + 1, LX = P * BX, LY = P * BY;
  const long plane = (long)NX * NY, ndofs = plane * NZ;
  // x: exactly ndofs doubles; shift 1: the block starts 8 bytes before x, so x is 8 bytes past a 16-byte boundary
  char* block = (char*)std::malloc((size_t)(ndofs + shift) * 8);
  if (shift) std::memset(block, 0xff, 8);
  char* const xb = block + 8 * shift;
  CHECK(((uintptr_t)xb & 15) == (uintptr_t)(8 * shift), "alignment of x");
  for (long d = 0; d < ndofs; ++d) {
    const double v = value_of(d);
    std::memcpy(xb + 8 * d, &v, 8);
  }
  const long lo = 0, hi = 8 * ndofs;   // byte range of the vector, relative to x

  const int nbx = (NX + LX - 1) / LX, nby = (NY + LY - 1) / LY;
  std::vector<int> count(R.RX * R.RY);
  std::vector<double> image(R.RX * R.RY);
  for (int By = 0; By < nby; ++By)
    for (int Bx = 0; Bx < nbx; ++Bx) {
      const int I0 = LX * Bx, J0 = LY * By;
      ++st.columns;
      int nstraddle = 0;
      // the planes of the first layer (0..P: the prologue) and of the last (P (nz - 1) + 1 .. P nz: the prefetch)
      for (int K = 0; K < NZ; ++K) {
        std::fill(count.begin(), count.end(), 0);
        std::fill(image.begin(), image.end(), 0.0);
        // pieces past the plane: 256 threads per plane slot of the kernel, two slots at 2 x 8
        for (int q = R.NPC; q < 512; ++q)
          CHECK(wf::owner_piece(P, BX, BY, NX, NY, I0, J0, q).kind == wf::PIECE_NONE, "piece %d past the plane", q);
        for (int q = 0; q < R.NPC; ++q) {
          const wf::OwnerPiece pc = wf::owner_piece(P, BX, BY, NX, NY, I0, J0, q);
          const long at = 8 * (plane * K + pc.off);
          if (pc.kind == wf::PIECE_INSIDE) {
            if (K == 0) ++st.inside;
            CHECK(at >= lo && at + 16 <= hi, "16-byte load at %ld of %ld (%dx%d, %dx%d, column %d,%d, plane %d, piece %d)", at, hi,
                  nx, ny, BX, BY, Bx, By, K, q);
            if (at >= lo && at + 16 <= hi) {
              std::memcpy(&image[2 * q], xb + at, 16);
              ++count[2 * q];
              ++count[2 * q + 1];
            }
          } else if (pc.kind == wf::PIECE_STRADDLING) {
            if (K == 0) ++st.straddling, ++nstraddle;
            CHECK(pc.half == 0, "straddling piece %d with its second position in the mesh", q);
            CHECK(at >= lo && at + 8 <= hi, "8-byte load at %ld of %ld (%dx%d, %dx%d, column %d,%d, plane %d, piece %d)", at, hi, nx,
                  ny, BX, BY, Bx, By, K, q);
            if (at >= lo && at + 8 <= hi && (pc.half == 0 || pc.half == 1)) {
              std::memcpy(&image[2 * q + pc.half], xb + at, 8);
              ++count[2 * q + pc.half];
            }
          } else {
            if (K == 0) ++st.outside;
            CHECK(pc.kind == wf::PIECE_OUTSIDE, "piece %d of kind %d", q, pc.kind);
          }
        }
        for (int r = 0; r < R.RY; ++r)
          for (int c = 0; c < R.RX; ++c) {
            const int II = I0 - P + c, JJ = J0 - P + r;
            const bool in = II >= 0 && II < NX && JJ >= 0 && JJ < NY;
            const int k = c + R.RX * r;
            if (in) {
              CHECK(count[k] == 1, "position (%d, %d) of the mesh filled %d times (%dx%d, %dx%d, column %d,%d, plane %d)", II, JJ,
                    count[k], nx, ny, BX, BY, Bx, By, K);
              CHECK(image[k] == value_of(II + (long)NX * JJ + plane * K), "position (%d, %d) holds another point's value", II, JJ);
            } else {
              CHECK(count[k] == 0, "position (%d, %d) outside the mesh loaded (%dx%d, %dx%d, column %d,%d, plane %d)", II, JJ, nx, ny,
                    BX, BY, Bx, By, K);
            }
          }
      }
      CHECK(nstraddle <= R.RY, "%d straddling pieces in a column of %d rows", nstraddle, R.RY);
    }
  std::free(block);
}

}  // namespace

int main()
{
  const int sizes[] = {1, 2, 7, 8, 9, 16, 17, 54};
  const int shapes[3][2] = {{4, 4}, {8, 2}, {2, 8}};
  static_assert(wf::owner_rect(4, 8, 2).RX == 38 && wf::owner_rect(4, 8, 2).NPC == 247, "8 x 2");
  static_assert(wf::owner_rect(4, 4, 4).RX == 22 && wf::owner_rect(4, 4, 4).NPC == 231, "4 x 4");
  static_assert(wf::owner_rect(4, 2, 8).RX == 14 && wf::owner_rect(4, 2, 8).NPC == 259, "2 x 8");
  for (const auto& s : shapes) {
    Stats st;
    for (int nx : sizes)
      for (int ny : sizes)
        for (int shift = 0; shift < 2; ++shift) walk(nx, ny, s[0], s[1], shift, st);
    std::printf("%d x %d: %ld columns, pieces inside %ld, straddling %ld, outside %ld\n", s[0], s[1], st.columns, st.inside,
                st.straddling, st.outside);
    if (st.inside == 0 || st.straddling == 0 || st.outside == 0) ++failures;   // every kind must have been met
  }
  std::printf("%ld failures\n", failures);
  return failures ? 1 : 0;
}
