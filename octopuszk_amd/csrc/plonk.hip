// The Fr side of the PLONK prover on gfx950 as one unit: the kernels, workspace layouts and C ABI (include/ozk.h) of
//   plonk.cuh         rows by coset powers, the permutation grand product, the quotient,
//   plonk_lookup.cuh  the lookup argument: index, counts, running sum, quotient (section 31),
//   plonk_r1cs.cuh    the witness on the device: running sums of a term stream, the gather of the wires (section 36),
//   plonk_zk.cuh      zero knowledge: the blinders of coefficient rows, the split of the quotient (section 37),
//   plonk_verify.cuh  the batched verifier: the transcripts and the scalars of K proofs (section 38),
// each a section of this unit.  What they share with the KZG unit is fr_rows.cuh's and fr_tables.cuh's; no kernel of
// kzg.hip is compiled here.
#include "plonk.cuh"
#include "plonk_lookup.cuh"
#include "plonk_r1cs.cuh"
#include "plonk_zk.cuh"
#include "plonk_verify.cuh"
