// tab_layout_check.cpp -- the table layout of saigegds_amd/csrc/host_tabs.h on its own, without HIP: built and run by
// tests/test_tab_layout.py with the host compiler under -fsanitize=address,undefined.  Every list of three slots over
// element sizes 1, 4, 8 and sizeof(SkatTile) and counts 0, 1, 15, 16, 17 is laid out, checked, and written and read
// through at<T>() in a heap buffer of exactly bytes() bytes, so that a slot that overruns is the sanitizer's to find.
#define TAB_LAYOUT_ONLY
#include "host_tabs.h"
#include <stdio.h>
#include <stdlib.h>

struct Tile { long long row_e0, col_e0; int nrow, ncol, dense, pad; };      // the shape of SkatTile (kern_skat.h)
static_assert(sizeof(Tile) == 32 && alignof(Tile) == 8, "Tile");

struct Any { int kind; size_t off, n, size; const void *src; };
static const size_t COUNTS[5] = {0, 1, 15, 16, 17};
static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { g_fail++; fprintf(stderr, "line %d: %s (list %d)\n", __LINE__, #c, list); } } while (0)

template <class T>
static Any put(TabLayout &tl, int kind, size_t n, const T *src)
{
	const TabSlot<T> s = tl.add<T>(n, src);
	return Any{kind, s.off, s.n, sizeof(T), s.src};
}

template <class T> static T value(size_t i, size_t e) { return (T)(i * 31 + e * 7 + 1); }
template <> Tile value<Tile>(size_t i, size_t e) { return Tile{(long long)i, (long long)e, 1, 2, 3, 4}; }
static bool same(const Tile &a, const Tile &b) { return a.row_e0 == b.row_e0 && a.col_e0 == b.col_e0 && a.pad == b.pad; }
template <class T> static bool same(const T &a, const T &b) { return a == b; }

template <class T>
static void write_all(uint8_t *base, const Any &a, size_t i)
{
	T *p = TabLayout::at(base, TabSlot<T>{a.off, a.n});
	for (size_t e = 0; e < a.n; e++) p[e] = value<T>(i, e);
}

template <class T>
static size_t read_bad(uint8_t *base, const Any &a, size_t i)
{
	const T *p = TabLayout::at(base, TabSlot<T>{a.off, a.n});
	size_t bad = 0;
	for (size_t e = 0; e < a.n; e++) bad += !same(p[e], value<T>(i, e));
	return bad;
}

int main()
{
	static const uint8_t host[17 * sizeof(Tile)] = {};      // a host source of any slot's size (never read here)
	for (int list = 0; list < 20 * 20 * 20; list++) {
		TabLayout tl;
		Any a[3];
		size_t sum = 0;
		for (int i = 0, code = list; i < 3; i++, code /= 20) {
			const int kind = code % 4;
			const size_t n = COUNTS[code % 20 / 4], before = tl.bytes();
			const bool src = (list + i) % 2 == 0;          // every other slot has a host source
			const void *sp = src ? host : nullptr;
			a[i] = kind == 0 ? put(tl, kind, n, (const uint8_t *)sp) : kind == 1 ? put(tl, kind, n, (const int32_t *)sp)
				: kind == 2 ? put(tl, kind, n, (const double *)sp) : put(tl, kind, n, (const Tile *)sp);
			sum += n * a[i].size;
			CHECK(a[i].src == sp && a[i].n == n);           // the slot keeps its count and its host source
			CHECK(a[i].off == before);                      // slots follow one another ...
			CHECK(a[i].off % 16 == 0);                      // ... each on a 16-byte boundary
			CHECK(a[i].off + n * a[i].size <= tl.bytes()); // inside bytes()
			CHECK(tl.bytes() - before < n * a[i].size + 16);   // at most the alignment more than its elements (n == 0: nothing)
			if (i) CHECK(a[i - 1].off + a[i - 1].n * a[i - 1].size <= a[i].off);   // no overlap
		}
		CHECK(tl.bytes() >= sum);

		uint8_t *base = (uint8_t *)malloc(tl.bytes());
		for (int pass = 0; pass < 2; pass++)
			for (size_t i = 0; i < 3; i++) {
				size_t bad = 0;
				switch (a[i].kind * 2 + pass) {
				case 0: write_all<uint8_t>(base, a[i], i); break;
				case 1: bad = read_bad<uint8_t>(base, a[i], i); break;
				case 2: write_all<int32_t>(base, a[i], i); break;
				case 3: bad = read_bad<int32_t>(base, a[i], i); break;
				case 4: write_all<double>(base, a[i], i); break;
				case 5: bad = read_bad<double>(base, a[i], i); break;
				case 6: write_all<Tile>(base, a[i], i); break;
				default: bad = read_bad<Tile>(base, a[i], i); break;
				}
				CHECK(bad == 0);                            // what a slot holds is what was written to it
			}
		free(base);
	}
	if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
	printf("tab layout: 8000 slot lists OK\n");
	return 0;
}
