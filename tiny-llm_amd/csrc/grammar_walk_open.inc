// What the walk of a lane's 8 tokens, c .. c + 7, opens with, whatever the automaton: included in the body of gr_walk8 (grammar.h) and of
// grs_walk8 (grammar_stack.h).  Shared as text and not as a function: the arrays it fills would cross the call by reference, and the
// regex walk then compiles to other code (24 more VGPRs, its light rows 6 % slower at 64 rows: profiles/grammar_refactor.json); as
// text, logit_process_kernel<true> stays instruction for instruction what it was.
//
// In scope where it is included: g (GrRef), c, vocab, offsets and bytes (the vocabulary's, through GR_GLOBAL), and the mode's long-token
// decision, a callable
//   long_ok(li) -> 1 where long token number li (long_index) can be walked from the row's state, else 0
// by the precomputed bit (regex) or depth byte (stack) of (state, token).  A long token is rare (a few hundred of the vocabulary) and
// is not a chain of the rounds.
// Leaves: off[e] .. off[e + 1] the bytes of token c + e, len[e] (0: not walked -- past the vocabulary, empty, or long), alive (bit e:
// chain e is walked), ok (bit e: token c + e can be walked; so far the long ones), cur[e] byte 0 of chain e.
int off[9];
if (c + 8 <= vocab) {  // (offsets is 256-byte aligned and c a multiple of 8: two 16-byte loads and one more entry)
    const auto o4 = reinterpret_cast<const u32x4 __attribute__((address_space(1))) *>(offsets + c);
    const u32x4 a = o4[0], b = o4[1];
    off[0] = a[0], off[1] = a[1], off[2] = a[2], off[3] = a[3], off[4] = b[0], off[5] = b[1], off[6] = b[2], off[7] = b[3];
    off[8] = offsets[c + 8];
} else {
#pragma unroll
    for (int e = 0; e < 9; ++e) off[e] = offsets[min(c + e, vocab)];
}
int len[8];
uint32_t cur[8];
uint32_t alive = 0u, ok = 0u;
#pragma unroll
for (int e = 0; e < 8; ++e) len[e] = c + e < vocab ? off[e + 1] - off[e] : 0;
uint32_t is_long = 0u;
#pragma unroll
for (int e = 0; e < 8; ++e) is_long |= len[e] > GR_LONG ? 1u << e : 0u;
if (is_long) {
    const auto long_index = GR_GLOBAL(int32_t, g.long_index);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (!(is_long >> e & 1u)) continue;
        ok |= long_ok(long_index[c + e]) << e;
        len[e] = 0;
    }
}
#pragma unroll
for (int e = 0; e < 8; ++e) alive |= len[e] > 0 ? 1u << e : 0u;
// (an empty token reads byte 0 of the buffer: in bounds, dropped)
#pragma unroll
for (int e = 0; e < 8; ++e) cur[e] = bytes[len[e] > 0 ? off[e] : 0];
