// Driver (ours) over the REFERENCE's transcript_set (rnacore/transcript_set.cc + gtf/transcript.cc), compiled against
// /root/reference sources.  It replays what assembler::assemble(gx, px, sid) does with the transcripts of each graph
// (meta/assembler.cc:1105-1133): per graph a local set `ts`, ts.add(t, 1, sid, ADD) for every transcript, then tm.add(ts, ADD).
// With the arguments `merge K1 K2 ...` (K1 + K2 + ... = G) the groups are cut into consecutive segments of K1, K2, ... groups, every
// segment is replayed into a transcript_set of its own, and the sets are folded left to right into the first with
// transcript_set::add(transcript_set&, TRANSCRIPT_COUNT_ADD_COVERAGE_ADD): two finished sets that both hold items.  The first set is printed.
// stdin:  G  then per graph "sid n" and n lines "strand coverage conf abd count1 nexons l r ... tid"
// stdout: every item of tm in map order:  hash count coverage cov2 conf abd count1 count2 tid nexons l r ... | nsamples {sid coverage cov2 conf abd count1 count2}
#include "transcript_set.h"
#include "constants.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
// one region replayed into tm: G groups read from stdin
static int replay(transcript_set &tm, int G)
{
	for(int g = 0; g < G; g++)
	{
		int sid, n;
		if(scanf("%d %d", &sid, &n) != 2) return 1;
		transcript_set ts("1", tm.rid, 0.8);
		for(int i = 0; i < n; i++)
		{
			char st; double cov, conf, abd; int c1, ne; char tid[64];
			if(scanf(" %c %lf %lf %lf %d %d", &st, &cov, &conf, &abd, &c1, &ne) != 6) return 1;
			transcript t;
			t.clear();
			t.seqname = "1"; t.strand = st; t.coverage = cov; t.cov2 = cov; t.conf = conf; t.abd = abd; t.count1 = c1; t.count2 = 1;
			for(int k = 0; k < ne; k++) { int l, r; if(scanf("%d %d", &l, &r) != 2) return 1; t.add_exon(l, r); }
			if(scanf("%63s", tid) != 1) return 1;
			t.transcript_id = tid; t.meta_tid = tid; t.RPKM = 0;
			ts.add(t, 1, sid, TRANSCRIPT_COUNT_ADD_COVERAGE_ADD);
		}
		tm.add(ts, TRANSCRIPT_COUNT_ADD_COVERAGE_ADD);
	}
	return 0;
}
int main(int argc, char **argv)
{
	int G;
	if(scanf("%d", &G) != 1) return 1;
	std::vector<int> seg;
	if(argc >= 2)
	{
		if(strcmp(argv[1], "merge") != 0 || argc < 3) return 2;
		long sum = 0;
		for(int a = 2; a < argc; a++) { int k = atoi(argv[a]); if(k < 0) return 2; seg.push_back(k); sum += k; }
		if(sum != G) return 2;
	}
	else seg.push_back(G);
	std::vector<transcript_set> sets;
	for(size_t s = 0; s < seg.size(); s++)
	{
		sets.push_back(transcript_set("1", 0, 0.8));
		if(replay(sets.back(), seg[s]) != 0) return 1;
	}
	transcript_set &tm = sets[0];
	for(size_t s = 1; s < sets.size(); s++) tm.add(sets[s], TRANSCRIPT_COUNT_ADD_COVERAGE_ADD);
	for(auto &x : tm.mt) for(auto &z : x.second)
	{
		const transcript &t = z.trst;
		printf("%lu %d %.17g %.17g %.17g %.17g %d %d %s %lu", x.first, z.count, t.coverage, t.cov2, t.conf, t.abd, t.count1, t.count2, t.transcript_id.c_str(), t.exons.size());
		for(auto &e : t.exons) printf(" %d %d", e.first, e.second);
		printf(" | %lu", z.samples.size());
		for(auto &s : z.samples) printf(" { %d %.17g %.17g %.17g %.17g %d %d }", s.first, s.second.coverage, s.second.cov2, s.second.conf, s.second.abd, s.second.count1, s.second.count2);
		printf("\n");
	}
	return 0;
}
