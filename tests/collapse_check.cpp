// collapse_check.cpp -- the checks of sgx_collapse_2bit's groups (saigegds_amd/csrc/host_collapse.h) on their own,
// without HIP: built and run by tests/test_collapse_ref.py with the host compiler under -fsanitize=address,undefined.
// Every list lives in a heap buffer of exactly its size, so that a check that reads beyond what a sound grp_ptr
// promises -- an entry past var_idx's end, a group past grp_ptr's -- is the sanitizer's to find.
#define COLLAPSE_CHECK_ONLY
#include "host_collapse.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { g_fail++; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

template <class T>
static T *exact(const std::vector<T> &v)                  // the elements in a block of exactly their bytes
{
	T *p = (T *)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
	if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
	return p;
}

// both steps as the entries run them: the indices are looked at only behind a sound grp_ptr
static int both(const std::vector<int64_t> &ptr, const std::vector<int32_t> &idx, size_t n_variants, size_t *at)
{
	int64_t *p = exact(ptr);
	int32_t *i = exact(idx);
	int rc = collapse_ptr_check(ptr.size() - 1, p, at);
	if (rc == COLLAPSE_OK) rc = collapse_idx_check((size_t)p[ptr.size() - 1], i, n_variants, at);
	free(p);
	free(i);
	return rc;
}

int main()
{
	size_t at = 99;
	CHECK(both({0, 2, 2, 5}, {0, 4, 4, 1, 0}, 5, &at) == COLLAPSE_OK);          // an empty group, a row in two groups
	CHECK(both({0}, {}, 0, &at) == COLLAPSE_OK);                                // no group
	CHECK(both({0, 0, 0}, {}, 0, &at) == COLLAPSE_OK);                          // empty groups, no rows
	CHECK(both({1, 2}, {0, 0}, 5, &at) == COLLAPSE_PTR0);
	CHECK(both({-1, 2}, {0, 0}, 5, &at) == COLLAPSE_PTR0);
	CHECK(both({0, 3, 2, 4}, {0, 0, 0, 0}, 5, &at) == COLLAPSE_DESCEND && at == 1);
	CHECK(both({0, -1}, {}, 5, &at) == COLLAPSE_DESCEND && at == 0);            // a negative end: nothing is indexed by it
	// an end far beyond var_idx with a descent behind it: the indices are never looked at
	CHECK(both({0, (int64_t)1 << 40, 1}, {0}, 5, &at) == COLLAPSE_DESCEND && at == 1);
	CHECK(both({0, 2, 3}, {0, 5, 1}, 5, &at) == COLLAPSE_INDEX && at == 1);     // n_variants itself is outside
	CHECK(both({0, 2, 3}, {0, 4, -1}, 5, &at) == COLLAPSE_INDEX && at == 2);
	CHECK(both({0, 1}, {0}, 0, &at) == COLLAPSE_INDEX && at == 0);              // no rows at all
	CHECK(both({0, 1}, {INT32_MIN}, 5, &at) == COLLAPSE_INDEX);
	CHECK(both({0, 1}, {INT32_MAX}, (size_t)INT32_MAX, &at) == COLLAPSE_INDEX);
	CHECK(both({0, 1}, {INT32_MAX}, (size_t)INT32_MAX + 1, &at) == COLLAPSE_OK);
	if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
	printf("collapse checks: 14 group lists OK\n");
	return 0;
}
