// The CPU side of the host-link leg: plain C++, no HIP call. The CPU
// fills a range of the pinned window with the march's pattern, or
// compares one with it, and records wrong words in the same
// HbmMarchResult the kernels use (count, lowest offset, the first 16 as
// {offset, expected, got, pass}). The leg calls these only after the
// launch or copy that touched the range has been synchronised.

// words[0, nwords) <- phase `phase` of the pattern; w0 is the logical
// word index of words[0].
static void host_pattern_fill(uint32_t* words, unsigned long long nwords,
                              unsigned long long w0, int phase) {
  if (phase == 2) {
    __builtin_memset(words, 0, nwords * sizeof(uint32_t));
    return;
  }
  const uint32_t flip = phase == 1 ? ~0u : 0u;
  for (unsigned long long i = 0; i < nwords; ++i)
    words[i] = hbm_march_pattern(w0 + i) ^ flip;
}

// Compare words[0, nwords) with phase `phase`; byte0 is the window byte
// offset of words[0]. Returns the number of wrong words found here.
static unsigned long long host_pattern_compare(const uint32_t* words,
                                               unsigned long long nwords,
                                               unsigned long long w0,
                                               unsigned long long byte0,
                                               int phase, int pass,
                                               HbmMarchResult* res) {
  const uint32_t flip = phase == 1 ? ~0u : 0u;
  unsigned long long bad = 0;
  for (unsigned long long i = 0; i < nwords; ++i) {
    const uint32_t want = phase == 2 ? 0u : hbm_march_pattern(w0 + i) ^ flip;
    const uint32_t got = words[i];
    if (got == want) continue;
    const unsigned long long off = byte0 + 4ull * i;
    if (off < res->first_bad_offset) res->first_bad_offset = off;
    const unsigned long long slot = res->mismatch_words++;
    if (slot < (unsigned long long)HBM_MARCH_RECORDS) {
      res->bad_offset[slot] = off;
      res->bad_expected[slot] = want;
      res->bad_got[slot] = got;
      res->bad_pass[slot] = pass;
    }
    ++bad;
  }
  return bad;
}

// `from`'s findings appended to `into`: counts add, the lower first
// offset wins, records fill the slots that are left.
static void host_pattern_merge(HbmMarchResult* into,
                               const HbmMarchResult& from) {
  unsigned long long have = into->mismatch_words < HBM_MARCH_RECORDS
                                ? into->mismatch_words
                                : HBM_MARCH_RECORDS;
  const unsigned long long n = from.mismatch_words < HBM_MARCH_RECORDS
                                   ? from.mismatch_words
                                   : HBM_MARCH_RECORDS;
  for (unsigned long long i = 0; i < n && have < HBM_MARCH_RECORDS;
       ++i, ++have) {
    into->bad_offset[have] = from.bad_offset[i];
    into->bad_expected[have] = from.bad_expected[i];
    into->bad_got[have] = from.bad_got[i];
    into->bad_pass[have] = from.bad_pass[i];
  }
  into->mismatch_words += from.mismatch_words;
  if (from.first_bad_offset < into->first_bad_offset)
    into->first_bad_offset = from.first_bad_offset;
}
