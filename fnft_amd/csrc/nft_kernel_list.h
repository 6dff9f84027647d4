// nft_kernel_list.h -- the one statement of which kernel templates are instantiated with which arguments.
//
// FA_LIST_<family>(X, ...) calls X(<arguments>, ...) once per member and hands the trailing arguments on; a consumer
// without any passes a dummy (FA_LIST_COL_N1(X, _)).  Three consumers read the lists:
//   - the dispatch switches of nft_dispatch.h build their case lines from them;
//   - the units FA_UNIT_<name>(I) below, one per hip_kernels_<name>.hip, apply I to every kernel functor of the unit
//     (I = FA_INST, hip_be.h: the explicit instantiation);
//   - the emulator's emu_kernel_list (tests/emu/emu_main.cpp) prints the names for the coverage tests.
// A new size goes into one list and is then dispatched, compiled and counted by the tests.
#pragma once

// ---- families ----------------------------------------------------------------------------------------------------
#define FA_LIST_BRIDGE_N1(X, ...) X(4, __VA_ARGS__) X(8, __VA_ARGS__) X(16, __VA_ARGS__) X(32, __VA_ARGS__) \
    X(64, __VA_ARGS__) X(128, __VA_ARGS__) X(256, __VA_ARGS__) X(512, __VA_ARGS__)
// KRColInv: up to 4096
#define FA_LIST_RCOL_INV_N1(X, ...) FA_LIST_BRIDGE_N1(X, __VA_ARGS__) X(1024, __VA_ARGS__) X(2048, __VA_ARGS__) X(4096, __VA_ARGS__)
// column lengths of the tree (KColFwd, KColInv): N1 = 2 would be a product of length 2*N2 <= 4096, which is fused (kFusedMaxN)
#define FA_LIST_COL_N1(X, ...) FA_LIST_RCOL_INV_N1(X, __VA_ARGS__) X(8192, __VA_ARGS__)
// the same lengths for a consumer whose X takes the length alone (the emulator's check of the column tilings)
#define FA_ARG1(n, X) X(n)
#define FA_FOR_EACH_N1(X) FA_LIST_COL_N1(FA_ARG1, X)
// KColBridge2: doubling transforms N1 points, not 2*N1
#define FA_LIST_BRIDGE2_N1(X, ...) FA_LIST_BRIDGE_N1(X, __VA_ARGS__) X(1024, __VA_ARGS__) X(2048, __VA_ARGS__) X(4096, __VA_ARGS__)
#define FA_LIST_CHIRP_N1(X, ...) X(2, __VA_ARGS__) FA_LIST_COL_N1(X, __VA_ARGS__)
// KPairFft, general form (NE = 4), in the three parts its units compile: fused up to N = 2048 (NftPlan::fused_max_len)
#define FA_LIST_PAIR_GEN_A(X, ...) X(8, __VA_ARGS__) X(16, __VA_ARGS__) X(32, __VA_ARGS__) X(64, __VA_ARGS__) X(128, __VA_ARGS__) X(256, __VA_ARGS__)
#define FA_LIST_PAIR_GEN_B(X, ...) X(512, __VA_ARGS__) X(1024, __VA_ARGS__)
#define FA_LIST_PAIR_GEN_C(X, ...) X(2048, __VA_ARGS__)
#define FA_LIST_PAIR_GEN(X, ...) FA_LIST_PAIR_GEN_A(X, __VA_ARGS__) FA_LIST_PAIR_GEN_B(X, __VA_ARGS__) FA_LIST_PAIR_GEN_C(X, __VA_ARGS__)
// KPairFft, symmetric form (NE = 2): starts at degree >= 6 (leaf kernel or coefficient program), so at N >= 16
#define FA_LIST_PAIR_SYM(X, ...) X(16, __VA_ARGS__) X(32, __VA_ARGS__) X(64, __VA_ARGS__) X(128, __VA_ARGS__) X(256, __VA_ARGS__) \
    X(512, __VA_ARGS__) X(1024, __VA_ARGS__) X(2048, __VA_ARGS__) X(4096, __VA_ARGS__)
// KMulti (N0, stages): the leaf kernel fused into the first launch (KLeafMulti) takes the levels from N = 16, so the
// launches that follow start at N = 128 and 1024
#define FA_LIST_MULTI3(X, ...) X(128, 3, __VA_ARGS__) X(1024, 3, __VA_ARGS__)
#define FA_LIST_MULTI2(X, ...) X(128, 2, __VA_ARGS__) X(1024, 2, __VA_ARGS__)
#define FA_LIST_MULTI(X, ...) FA_LIST_MULTI3(X, __VA_ARGS__) FA_LIST_MULTI2(X, __VA_ARGS__)
// KLeafMulti (deg, stages)
#define FA_LIST_LEAF_MULTI(X, ...) X(1, 3, __VA_ARGS__) X(2, 3, __VA_ARGS__) X(4, 3, __VA_ARGS__) \
    X(1, 2, __VA_ARGS__) X(2, 2, __VA_ARGS__) X(4, 2, __VA_ARGS__)
// the first FFT level of the real path has M >= 8; KRPair4 takes M = 32 ... 512
#define FA_LIST_RPAIR_M(X, ...) X(8, __VA_ARGS__) X(16, __VA_ARGS__) X(1024, __VA_ARGS__) X(2048, __VA_ARGS__)
#define FA_LIST_RPAIR4_M(X, ...) X(32, __VA_ARGS__) X(64, __VA_ARGS__) X(128, __VA_ARGS__) X(256, __VA_ARGS__) X(512, __VA_ARGS__)
// a forward column step of the real path runs on the first split level, whose length is the first above the fused
// limit (N1 = 4), and after a level without a bridge, which only the bridge limit kRBridgeMaxN1 causes (KRColInv<2048>,
// then KRColFwd<4096>)
#define FA_LIST_RCOL_FWD_N1(X, ...) X(4, __VA_ARGS__) X(4096, __VA_ARGS__)
#define FA_LIST_RBRIDGE_N1(X, ...) FA_LIST_BRIDGE_N1(X, __VA_ARGS__) X(1024, __VA_ARGS__)
// radix-3 columns of length 3*K.  Forward: only the first split level (K = 1): a level without a bridge (K = 512) is the last
#define FA_LIST_R3_FWD_K(X, ...) X(1, __VA_ARGS__)
#define FA_LIST_R3_BRIDGE_K(X, ...) X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(4, __VA_ARGS__) X(8, __VA_ARGS__) X(16, __VA_ARGS__) \
    X(32, __VA_ARGS__) X(64, __VA_ARGS__) X(128, __VA_ARGS__) X(256, __VA_ARGS__)
#define FA_LIST_R3_INV_K(X, ...) FA_LIST_R3_BRIDGE_K(X, __VA_ARGS__) X(512, __VA_ARGS__)
#define FA_LIST_COEFFS_DEG(X, ...) X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__)
#define FA_LIST_LEAF_DEG(X, ...) X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__)
#define FA_LIST_SCHOOL_DEG(X, ...) X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__)
// no d = 3 on the real path: the leaf kernel starts a tree of degree-3 factors at d = 6
#define FA_LIST_RSCHOOL_DEG(X, ...) X(1, __VA_ARGS__) X(2, __VA_ARGS__)
// KRCoeffsStrang, KRLeafStrang (akns_disc; order, bfirst): 13 (2SPLIT6A), 14 (6B), 17 (8A), 18 (8B)
#define FA_LIST_RSTRANG(X, ...) X(13, 6, false, __VA_ARGS__) X(14, 6, true, __VA_ARGS__) X(17, 8, false, __VA_ARGS__) X(18, 8, true, __VA_ARGS__)
#define FA_LIST_PEEL_N(X, ...) X(512, __VA_ARGS__) X(1024, __VA_ARGS__) X(2048, __VA_ARGS__)
#define FA_LIST_MIDGEN_N2(X, ...) X(1024, __VA_ARGS__) X(2048, __VA_ARGS__)   // kRowGen, kRowTree
// KSlowScatter (fam, realk): fam 0 CF family, 1 ES4, 2 TES4; realk: the CF family's real-ks variant
#define FA_LIST_SLOW_SCATTER(X, ...) X(0, true, __VA_ARGS__) X(0, false, __VA_ARGS__) X(1, false, __VA_ARGS__) X(2, false, __VA_ARGS__)
// KBsChunk, KBsCombine, KDsNewton, KDsNorm; KMidSym<DIRECT> in the order its unit has always had
#define FA_LIST_BOOL(X, ...) X(false, __VA_ARGS__) X(true, __VA_ARGS__)
#define FA_LIST_MIDSYM(X, ...) X(true, __VA_ARGS__) X(false, __VA_ARGS__)

// ---- list member -> kernel functor, for the units: I(K<n>), I(K<n, trailing...>), I(K<a, b>) ----------------------
#define FA_K1(n, I, K) I(K<n>)
#define FA_K1A(n, I, K, ...) I(K<n, __VA_ARGS__>)
#define FA_K2(a, b, I, K) I(K<a, b>)
#define FA_KSTRANG(disc, order, bfirst, I, K) I(K<order, bfirst>)

// ---- units: members and order of hip_kernels_<name>.hip (the grouping balances compile time) -----------------------
#define FA_UNIT_misc(I) \
    FA_LIST_COEFFS_DEG(FA_K1, I, KCoeffs) I(KCoeffsProg) I(KResamplePhase) I(KResampleCombine) I(KBandCheck) \
    FA_LIST_BOOL(FA_K1, I, KBsChunk) FA_LIST_BOOL(FA_K1, I, KBsCombine) I(KBsPhi) I(KBsMetric) I(KBsPick) I(KBsPsi) \
    I(KBsMatrix) I(KGridMark) I(KGridMarkPh) I(KCompactCount) I(KCompactScatter) I(KInvOp) I(KInvSolitons) I(KInvCdt) \
    I(KInvDsPrep) I(KPeelImport) I(KPeelLeaf) FA_LIST_PEEL_N(FA_K1, I, KPeelProduct) I(KAberthNewton) I(KAberthSum) \
    I(KAberthApply) I(KFinalizeScales) I(KExportTm) I(KImportLevel0) FA_LIST_LEAF_DEG(FA_K1, I, KLeaf) \
    FA_LIST_SCHOOL_DEG(FA_K1, I, KPairSchool)
#define FA_UNIT_pair4a(I) FA_LIST_PAIR_GEN_A(FA_K1A, I, KPairFft, 4)
#define FA_UNIT_pair4b(I) FA_LIST_PAIR_GEN_B(FA_K1A, I, KPairFft, 4)
#define FA_UNIT_pair4c(I) FA_LIST_PAIR_GEN_C(FA_K1A, I, KPairFft, 4)
#define FA_UNIT_pair2(I) FA_LIST_PAIR_SYM(FA_K1A, I, KPairFft, 2)
#define FA_UNIT_multi3(I) FA_LIST_MULTI3(FA_K2, I, KMulti)
#define FA_UNIT_multi2(I) FA_LIST_MULTI2(FA_K2, I, KMulti)
#define FA_UNIT_leafmulti(I) FA_LIST_LEAF_MULTI(FA_K2, I, KLeafMulti)
#define FA_UNIT_discbatch(I) I(KDsBox) FA_LIST_BOOL(FA_K1, I, KDsNewton) I(KDsFilter) FA_LIST_BOOL(FA_K1, I, KDsNorm)
#define FA_UNIT_discroots(I) \
    I(KDsGather) I(KAberthBStart) I(KAberthBNewton) I(KAberthBSum) I(KAberthBApply) I(KAberthBStep) I(KDsCandidates)
#define FA_UNIT_slow(I) I(KSlowPrep) FA_LIST_SLOW_SCATTER(FA_K2, I, KSlowScatter) I(KSlowReduce) I(KSlowCombine)
#define FA_UNIT_mid(I) FA_LIST_MIDSYM(FA_K1, I, KMidSym)
#define FA_UNIT_col(I) FA_LIST_COL_N1(FA_K1, I, KColFwd) FA_LIST_COL_N1(FA_K1, I, KColInv)
#define FA_UNIT_bridge(I) FA_LIST_BRIDGE2_N1(FA_K1, I, KColBridge2)
#define FA_UNIT_realpair(I) \
    I(KRealCheck) FA_LIST_RSTRANG(FA_KSTRANG, I, KRCoeffsStrang) FA_LIST_RSCHOOL_DEG(FA_K1, I, KRPairSchool) \
    FA_LIST_RPAIR_M(FA_K1, I, KRPair)
#define FA_UNIT_realpair4(I) FA_LIST_RPAIR4_M(FA_K1, I, KRPair4)
#define FA_UNIT_realcol(I) FA_LIST_RCOL_FWD_N1(FA_K1, I, KRColFwd) FA_LIST_RCOL_INV_N1(FA_K1, I, KRColInv)
#define FA_UNIT_realbridge(I) FA_LIST_RBRIDGE_N1(FA_K1, I, KRBridge) FA_LIST_MIDGEN_N2(FA_K1, I, KMidGen)
#define FA_UNIT_real3col(I) FA_LIST_R3_FWD_K(FA_K1, I, KR3ColFwd) FA_LIST_R3_INV_K(FA_K1, I, KR3ColInv)
#define FA_UNIT_real3bridge(I) FA_LIST_R3_BRIDGE_K(FA_K1, I, KR3Bridge)
#define FA_UNIT_realleaf(I) FA_LIST_RSTRANG(FA_KSTRANG, I, KRLeafStrang)
#define FA_UNIT_chirpa(I) \
    I(KChirpRows) FA_LIST_CHIRP_N1(FA_K1A, I, KChirpColFwd, false) FA_LIST_CHIRP_N1(FA_K1A, I, KChirpColFwd, true)
#define FA_UNIT_chirpb(I) \
    FA_LIST_CHIRP_N1(FA_K1A, I, KChirpColInv, false, false) FA_LIST_CHIRP_N1(FA_K1A, I, KChirpColInv, true, false) \
    FA_LIST_CHIRP_N1(FA_K1A, I, KChirpColInv, false, true)
#define FA_UNIT_polyeval(I) FA_LIST_BOOL(FA_K1, I, KPolyEval) I(KPolyJoin)
#define FA_UNIT_richardson(I) I(KRichCombineCs) I(KRichMatchDs)
// every unit of the count the tests pin (258 kernels in 23 units), in the order of the file names
#define FA_ALL_UNITS(I) \
    FA_UNIT_bridge(I) FA_UNIT_chirpa(I) FA_UNIT_chirpb(I) FA_UNIT_col(I) FA_UNIT_discbatch(I) FA_UNIT_discroots(I) \
    FA_UNIT_leafmulti(I) FA_UNIT_mid(I) FA_UNIT_misc(I) FA_UNIT_multi2(I) FA_UNIT_multi3(I) FA_UNIT_pair2(I) \
    FA_UNIT_pair4a(I) FA_UNIT_pair4b(I) FA_UNIT_pair4c(I) FA_UNIT_real3bridge(I) FA_UNIT_real3col(I) \
    FA_UNIT_realbridge(I) FA_UNIT_realcol(I) FA_UNIT_realleaf(I) FA_UNIT_realpair(I) FA_UNIT_realpair4(I) FA_UNIT_slow(I)
// the units added after that count was pinned.  A unit is in exactly one of the three aggregates; together they are
// every hip_kernels_<name>.hip
#define FA_EXT_UNITS(I) FA_UNIT_polyeval(I)
// the units added after the tests pinned FA_EXT_UNITS to the polynomial evaluation
#define FA_EXT2_UNITS(I) FA_UNIT_richardson(I)
