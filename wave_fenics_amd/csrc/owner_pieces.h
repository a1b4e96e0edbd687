// Owner stiffness kernel, P = 4 ("r25"): the staged rectangle of one x plane in 16-byte pieces.
//
// The rectangle of a column holds the lattice positions (I0 - P + c, J0 - P + r), c in [0, RX), r in [0, RY), row
// stride RX.  RX is the parent's LX + P + 1 made even (one pad position per row), so a row is RX / 2 pieces of two
// x-consecutive positions and a plane is RX RY / 2 of them, piece q at the doubles 2q, 2q + 1 of the plane's LDS image.
// Thread q % 256 of the workgroup owns piece q of every plane.  A piece is classified once per run:
//   inside     both positions are in the mesh: one 16-byte direct-to-LDS load (the source is only 8-byte aligned);
//   outside    neither is: never loaded, its two doubles are set to +0.0 once;
//   straddling one is, one is not (the mesh's last lattice line in x, as NX is odd and a piece starts at an even
//              lattice index): an 8-byte load and an 8-byte LDS store for the one that is, its partner set to +0.0 once.
// Plain inline functions: the kernel and the host program tests/cxx/owner_pieces_walk.cpp both use them.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WF_PIECE_FN __host__ __device__ inline
#else
#define WF_PIECE_FN inline
#endif

namespace wf {

enum OwnerPieceKind { PIECE_NONE = 0, PIECE_OUTSIDE = 1, PIECE_INSIDE = 2, PIECE_STRADDLING = 3 };

struct OwnerRect {
  int RX, RY, NPC;   // row stride (even), rows, pieces of one plane
};
constexpr OwnerRect owner_rect(int P, int BX, int BY)
{
  const int rx = P * BX + P + 1, RX = rx + (rx & 1), RY = P * BY + P + 1;
  return {RX, RY, RX * RY / 2};
}

struct OwnerPiece {
  int kind;   // OwnerPieceKind; PIECE_NONE: q is past the plane
  int half;   // straddling: which of the piece's two positions is in the mesh
  int off;    // inside: lattice offset of the first position within its plane; straddling: of the one in the mesh
};

// Piece q of the column whose first owned line is (I0, J0), on a lattice of NX x NY lines per plane.
WF_PIECE_FN OwnerPiece owner_piece(int P, int BX, int BY, int NX, int NY, int I0, int J0, int q)
{
  const OwnerRect R = owner_rect(P, BX, BY);
  OwnerPiece p = {PIECE_NONE, 0, 0};
  if (q < 0 || q >= R.NPC) return p;
  const int hr = R.RX / 2, II = I0 - P + 2 * (q % hr), JJ = J0 - P + q / hr;
  const bool row = JJ >= 0 && JJ < NY;
  const bool in0 = row && II >= 0 && II < NX, in1 = row && II + 1 >= 0 && II + 1 < NX;
  if (in0 && in1) {
    p.kind = PIECE_INSIDE;
    p.off = II + NX * JJ;
  } else if (in0 || in1) {
    p.kind = PIECE_STRADDLING;
    p.half = in1 ? 1 : 0;
    p.off = II + p.half + NX * JJ;
  } else {
    p.kind = PIECE_OUTSIDE;
  }
  return p;
}

}  // namespace wf
