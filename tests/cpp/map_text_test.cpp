// The text of the map family (deacon-server_amd/cli/map_text.hpp) against strings written by hand from the rules that the
// help texts and include/*.h state.  Stand-alone: no device, no library; built with the sanitizers by tests/test_map_text.py.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "map_text.hpp"

static int bad = 0, checks = 0;
static void same(const char *what, const std::string &got, const std::string &want) {
    ++checks;
    if (got == want) return;
    ++bad;
    std::printf("FAIL %s\n  got  [%s]\n  want [%s]\n", what, got.c_str(), want.c_str());
}
static void same(const char *what, uint64_t got, uint64_t want) { same(what, std::to_string(got), std::to_string(want)); }

static void test_genotype_alleles() {
    const unsigned diploid[10][2] = {{0, 0}, {0, 1}, {1, 1}, {0, 2}, {1, 2}, {2, 2}, {0, 3}, {1, 3}, {2, 3}, {3, 3}};
    for (unsigned gt = 0; gt < 10; ++gt) {
        const GenotypeAlleles a = genotype_alleles(gt, 2);
        same("diploid x", a.x, diploid[gt][0]);
        same("diploid y", a.y, diploid[gt][1]);
    }
    for (unsigned gt = 0; gt < 4; ++gt) {
        const GenotypeAlleles a = genotype_alleles(gt, 1);
        same("haploid x", a.x, gt);
        same("haploid y", a.y, gt);
    }
}

static dcn_genotype_site site(unsigned gt, unsigned ref_code, const uint32_t (&ad)[4], const uint8_t (&pl)[10]) {
    dcn_genotype_site g = {};
    g.pos = 99, g.qual = 50, g.depth = 30, g.gt = (uint8_t)gt, g.gq = 40, g.ref_code = (uint8_t)ref_code;
    std::memcpy(g.ad, ad, sizeof ad);
    std::memcpy(g.pl, pl, sizeof pl);
    return g;
}

static void test_snv_lines() {
    // G3's order: AA AC CC AG CG GG AT CT GT TT
    const uint8_t pl[10] = {90, 91, 92, 93, 94, 95, 96, 97, 0, 99};
    const uint32_t ad2[4] = {10, 0, 20, 0}, ad3[4] = {1, 2, 3, 4};
    std::string s;
    append_snv_line(s, "chr1", site(5, 0, ad2, pl), 2); // G/G on A
    same("hom-alt", s, "chr1\t100\t.\tA\tG\t50\tPASS\tDP=30\tGT:GQ:DP:AD:PL\t1/1:40:30:10,20:90,93,95\n");
    s.clear();
    append_snv_line(s, "chr1", site(3, 0, ad2, pl), 2); // A/G on A
    same("het ref/alt", s, "chr1\t100\t.\tA\tG\t50\tPASS\tDP=30\tGT:GQ:DP:AD:PL\t0/1:40:30:10,20:90,93,95\n");
    s.clear();
    append_snv_line(s, "chr1", site(3, 2, ad2, pl), 2); // A/G on G: the record's base is REF, A the one ALT
    same("het alt/ref", s, "chr1\t100\t.\tG\tA\t50\tPASS\tDP=30\tGT:GQ:DP:AD:PL\t0/1:40:30:20,10:95,93,90\n");
    s.clear();
    append_snv_line(s, "chr1", site(8, 0, ad3, pl), 2); // G/T on A: three alleles, PL over (A, G, T) in VCF's order
    same("het alt/alt", s, "chr1\t100\t.\tA\tG,T\t50\tPASS\tDP=30\tGT:GQ:DP:AD:PL\t1/2:40:10:1,3,4:90,93,95,96,0,99\n");
    s.clear();
    append_snv_line(s, "chr1", site(2, 0, ad2, pl), 1); // G on A, haploid: a PL per allele
    same("haploid", s, "chr1\t100\t.\tA\tG\t50\tPASS\tDP=30\tGT:GQ:DP:AD:PL\t1:40:30:10,20:90,92\n");

    dcn_strand_site st = {};
    const uint32_t fwd[4] = {6, 0, 11, 0}, rev[4] = {4, 0, 9, 0};
    std::memcpy(st.fwd, fwd, sizeof fwd);
    std::memcpy(st.rev, rev, sizeof rev);
    st.sb_centi = 1234, st.flags = DCN_STRAND_BIAS;
    s.clear();
    append_snv_line(s, "chr1", site(3, 0, ad2, pl), 2, &st);
    same("strand", s, "chr1\t100\t.\tA\tG\t50\tstrand_bias\tDP=30;SB=12.34\tGT:GQ:DP:AD:ADF:ADR:PL\t0/1:40:30:10,20:6,11:4,9:90,93,95\n");
    st.sb_centi = 5, st.flags = 0;
    same("PASS", strand_filter(st), "PASS");
    same("SB 0.05", strand_sb(st), "0.05");
    st.flags = DCN_STRAND_ONE_SIDED;
    same("one_strand", strand_filter(st), "one_strand");
    st.flags = DCN_STRAND_BIAS | DCN_STRAND_ONE_SIDED;
    same("both filters", strand_filter(st), "strand_bias;one_strand");

    // phased: haplotype 1 carries a[hap], PS is the POS of the set's first site
    st.flags = 0;
    dcn_phase_site ps = {};
    ps.pos = 99, ps.a0 = 0, ps.a1 = 2;
    dcn_phase_result ph = {};
    ph.set_pos = 41, ph.flags = DCN_PHASE_JOINED;
    for (unsigned hap = 0; hap < 2; ++hap) {
        ph.hap = (uint8_t)hap;
        s.clear();
        append_snv_line(s, "chr1", site(3, 0, ad2, pl), 2, &st, &ps, &ph);
        same("phased", s, std::string("chr1\t100\t.\tA\tG\t50\tPASS\tDP=30;SB=0.05\tGT:GQ:DP:AD:ADF:ADR:PL:PS\t") + (hap ? "1|0" : "0|1") +
                              ":40:30:10,20:6,11:4,9:90,93,95:42\n");
    }
    // the list entry of a heterozygous site: a0 the record's base when the genotype holds it, else the lower column
    dcn_phase_site made;
    same("hom is no phase site", phase_site_of(site(5, 0, ad2, pl), 2, 3, made), 0);
    same("het is one", phase_site_of(site(3, 2, ad2, pl), 2, 3, made), 1);
    same("a0 = ref", made.a0, 2), same("a1", made.a1, 0), same("record", made.record, 3), same("pos", made.pos, 99);
    phase_site_of(site(8, 0, ad3, pl), 2, 0, made);
    same("a0 = lower", made.a0, 2), same("a1 = upper", made.a1, 3);
    const dcn_strand_query q = snv_strand_query(site(8, 0, ad3, pl), 2);
    same("ALT mask", q.alt_mask, (1u << 2) | (1u << 3)), same("query pos", q.pos, 99), same("query ref", q.ref_code, 0);
    same("ALT mask without REF", snv_strand_query(site(3, 0, ad2, pl), 2).alt_mask, 1u << 2);
    same("haploid ALT mask", snv_strand_query(site(2, 0, ad2, pl), 1).alt_mask, 1u << 2);
}

static void test_indel_lines() {
    const std::string record = "ACGTACGTAC";
    const uint64_t start = 2, n = 6; // the stretch holds GTACGT
    int fetched = 0;
    const auto fetch = [&](uint64_t from, uint64_t count) {
        ++fetched;
        return record.substr(from, count);
    };
    const auto ref_bases = [&](uint64_t from, uint64_t count) {
        return reference_bases((const uint8_t *)record.data() + start, start, n, from, count, fetch);
    };
    const uint8_t ins[] = {'G', 'G', 'T', 'T'};
    dcn_indel_site s = {};
    s.qual = 77, s.depth = 20, s.count = 8, s.events = 9, s.gq = 33, s.pl[0] = 50, s.pl[1] = 0, s.pl[2] = 60;
    std::string out;
    const auto line = [&](unsigned ploidy, const dcn_strand_site *st = nullptr) {
        const IndelAlleles v = indel_alleles(s, ins, ref_bases);
        out.clear();
        append_indel_line(out, "chr1", v, s, ploidy, st);
        return v.pos1;
    };
    // a deletion of AC at 4: anchored on the T before it
    s.pos = 4, s.len = 2, s.flags = DCN_INDEL_DELETION, s.gt = 1;
    same("deletion POS", line(2), 4);
    same("deletion het", out, "chr1\t4\t.\tTAC\tT\t77\tPASS\tINDEL;DP=20;IDV=8;IEV=9\tGT:GQ:DP:AD:PL\t0/1:33:20:12,8:50,0,60\n");
    same("inside the stretch", fetched, 0);
    s.gt = 2;
    line(2);
    same("deletion hom", out, "chr1\t4\t.\tTAC\tT\t77\tPASS\tINDEL;DP=20;IDV=8;IEV=9\tGT:GQ:DP:AD:PL\t1/1:33:20:12,8:50,0,60\n");
    // a deletion of AC at 0: there is no base before it, the base behind is the anchor (and lies outside the stretch)
    s.pos = 0;
    same("deletion at 0 POS", line(2), 1);
    same("deletion at 0", out, "chr1\t1\t.\tACG\tG\t77\tPASS\tINDEL;DP=20;IDV=8;IEV=9\tGT:GQ:DP:AD:PL\t1/1:33:20:12,8:50,0,60\n");
    same("fetched beyond the stretch", fetched, 1);
    // a deletion that begins in the stretch and ends behind it
    s.pos = 6, s.len = 3;
    line(2);
    same("deletion over the seam", out, "chr1\t6\t.\tCGTA\tC\t77\tPASS\tINDEL;DP=20;IDV=8;IEV=9\tGT:GQ:DP:AD:PL\t1/1:33:20:12,8:50,0,60\n");
    same("fetched over the seam", fetched, 2);
    // GG behind the C at 5
    s.pos = 5, s.len = 2, s.flags = 0, s.bases_offset = 0, s.gt = 1;
    same("insertion POS", line(2), 6);
    same("insertion behind", out, "chr1\t6\t.\tC\tCGG\t77\tPASS\tINDEL;DP=20;IDV=8;IEV=9\tGT:GQ:DP:AD:PL\t0/1:33:20:12,8:50,0,60\n");
    // TT in front of the T at 3: behind the G at 2
    s.pos = 3, s.flags = DCN_INDEL_FRONT, s.bases_offset = 2;
    same("front POS", line(2), 3);
    same("insertion in front", out, "chr1\t3\t.\tG\tGTT\t77\tPASS\tINDEL;DP=20;IDV=8;IEV=9\tGT:GQ:DP:AD:PL\t0/1:33:20:12,8:50,0,60\n");
    // TT in front of the record's first base
    s.pos = 0;
    same("front at 0 POS", line(2), 1);
    same("insertion in front at 0", out, "chr1\t1\t.\tA\tTTA\t77\tPASS\tINDEL;DP=20;IDV=8;IEV=9\tGT:GQ:DP:AD:PL\t0/1:33:20:12,8:50,0,60\n");
    same("fetched in front of the stretch", fetched, 3);
    // haploid: the allele, and two likelihoods
    s.pos = 5, s.flags = 0, s.bases_offset = 0, s.gt = 1;
    line(1);
    same("haploid", out, "chr1\t6\t.\tC\tCGG\t77\tPASS\tINDEL;DP=20;IDV=8;IEV=9\tGT:GQ:DP:AD:PL\t1:33:20:12,8:50,0\n");
    same("haploid is hom", indel_is_hom(s, 1), 1);
    same("diploid het", indel_is_hom(s, 2), 0);
    // the strand table a b c d: others forward, others reverse, allele forward, allele reverse
    dcn_strand_site st = {};
    st.table[0] = 7, st.table[1] = 5, st.table[2] = 3, st.table[3] = 5, st.sb_centi = 5, st.flags = DCN_STRAND_ONE_SIDED;
    s.gt = 2;
    line(2, &st);
    same("strand", out, "chr1\t6\t.\tC\tCGG\t77\tone_strand\tINDEL;DP=20;IDV=8;IEV=9;SB=0.05\tGT:GQ:DP:AD:ADF:ADR:PL\t1/1:33:20:12,8:7,3:5,5:50,0,60\n");
    // more reads with the allele than depth: no negative count
    s.count = 25;
    line(2);
    same("count above depth", out, "chr1\t6\t.\tC\tCGG\t77\tPASS\tINDEL;DP=20;IDV=25;IEV=9\tGT:GQ:DP:AD:PL\t1/1:33:25:0,25:50,0,60\n");
}

static void test_block_lines() {
    dcn_reference_block b = {};
    b.pos = 10, b.len = 5, b.sum_depth = 44, b.min_depth = 7, b.max_depth = 12, b.min_gq = 35, b.cls = DCN_BLOCK_REF + 2;
    std::string s;
    append_block_line(s, "chr1", b, 'c', 2);
    same("REF diploid", s, "chr1\t11\t.\tC\t<NON_REF>\t.\t.\tEND=15\tGT:GQ:DP:MIN_DP\t0/0:35:8:7\n"); // 44 / 5, rounded down
    s.clear();
    append_block_line(s, "chr1", b, 'C', 1);
    same("REF haploid", s, "chr1\t11\t.\tC\t<NON_REF>\t.\t.\tEND=15\tGT:GQ:DP:MIN_DP\t0:35:8:7\n");
    b.cls = DCN_BLOCK_UNCALLED;
    s.clear();
    append_block_line(s, "chr1", b, 'G', 2);
    same("not called diploid", s, "chr1\t11\t.\tG\t<NON_REF>\t.\t.\tEND=15\tGT:GQ:DP:MIN_DP\t./.:35:8:7\n");
    b.cls = DCN_BLOCK_NO_COVERAGE, b.sum_depth = 0, b.min_depth = 0, b.min_gq = 0;
    s.clear();
    append_block_line(s, "chr1", b, 'G', 1);
    same("no coverage haploid", s, "chr1\t11\t.\tG\t<NON_REF>\t.\t.\tEND=15\tGT:GQ:DP:MIN_DP\t.:0:0:0\n");
}

// `lines` behind the first line of `head` that begins with `after`
static std::string with_lines(const std::string &head, const std::string &after, const std::string &lines) {
    size_t at = head.find("\n" + after);
    if (at == std::string::npos) return "no line " + after;
    at = head.find('\n', at + 1) + 1;
    return head.substr(0, at) + lines + head.substr(at);
}

static void test_headers() {
    const std::vector<std::string> names = {"chr1", "chr2"};
    const std::vector<uint32_t> lens = {10, 20};
    const std::string genotype =
        "##fileformat=VCFv4.2\n##source=deacon-hip 9.9\n##contig=<ID=chr1,length=10>\n##contig=<ID=chr2,length=20>\n"
        "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth: reads with a base, an N or a deletion at the position\">\n"
        "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
        "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: phred gap to the second best genotype, at most 99\">\n"
        "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Bases A, C, G, T of at least the minimum base quality\">\n"
        "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Such bases per allele\">\n"
        "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods, at most 255\">\n";
    VcfModes m;
    same("genotype and markdup", vcf_header("9.9", m, names, lens), genotype);
    m.indels = true; // three INFO keys behind DP
    const std::string indels = with_lines(genotype, "##INFO=<ID=DP,",
        "##INFO=<ID=INDEL,Number=0,Type=Flag,Description=\"An insertion or a deletion\">\n"
        "##INFO=<ID=IDV,Number=1,Type=Integer,Description=\"Reads that carry the allele\">\n"
        "##INFO=<ID=IEV,Number=1,Type=Integer,Description=\"Insertions behind, or deletions that begin at, the position, of any allele\">\n");
    same("indels", vcf_header("9.9", m, names, lens), indels);
    m.normalize = true; // one line that says so
    const std::string normalize = with_lines(indels, "##INFO=<ID=IEV,", "##left_aligned=The positions of insertions and deletions are left-aligned per read\n");
    same("normalize", vcf_header("9.9", m, names, lens), normalize);
    m.strand = true; // two FILTERs, SB, ADF and ADR
    std::string strand = with_lines(normalize, "##contig=<ID=chr2,",
        "##FILTER=<ID=strand_bias,Description=\"SB at or above --max-sb: the allele and the strand are not independent\">\n"
        "##FILTER=<ID=one_strand,Description=\"Both strands cover the site, the allele is on fewer than --min-alt-strand reads of one\">\n");
    strand = with_lines(strand, "##INFO=<ID=DP,",
        "##INFO=<ID=SB,Number=1,Type=Float,Description=\"Strand bias: chi-square of the 2 x 2 table of allele by strand, one degree of freedom\">\n");
    strand = with_lines(strand, "##FORMAT=<ID=AD,",
        "##FORMAT=<ID=ADF,Number=R,Type=Integer,Description=\"AD on the forward strand\">\n"
        "##FORMAT=<ID=ADR,Number=R,Type=Integer,Description=\"AD on the reverse strand\">\n");
    same("strand and gvcf's --vcf", vcf_header("9.9", m, names, lens), strand);
    m.phase = true; // PS
    same("phase", vcf_header("9.9", m, names, lens), with_lines(strand, "##FORMAT=<ID=PL,",
        "##FORMAT=<ID=PS,Number=1,Type=Integer,Description=\"Phase set: POS of the first site of the set the genotype is phased in\">\n"));
    // --gvcf: what the block lines use, then a band per edge and one on either side
    const std::string blocks =
        "##ALT=<ID=NON_REF,Description=\"Any allele other than the reference's: the line is a reference block\">\n"
        "##INFO=<ID=END,Number=1,Type=Integer,Description=\"Last position of the block\">\n"
        "##FORMAT=<ID=MIN_DP,Number=1,Type=Integer,Description=\"Smallest DP of the block's positions\">\n";
    same("default bands", gvcf_header_lines(CallOptions().gq_bands), blocks +
        "##GVCFBlock0-20=minGQ=0(inclusive),maxGQ=20(exclusive)\n##GVCFBlock20-40=minGQ=20(inclusive),maxGQ=40(exclusive)\n"
        "##GVCFBlock40-60=minGQ=40(inclusive),maxGQ=60(exclusive)\n##GVCFBlock60-80=minGQ=60(inclusive),maxGQ=80(exclusive)\n"
        "##GVCFBlock80-99=minGQ=80(inclusive),maxGQ=99(exclusive)\n##GVCFBlock99-100=minGQ=99(inclusive),maxGQ=100(exclusive)\n");
    same("one band", gvcf_header_lines({30}), blocks +
        "##GVCFBlock0-30=minGQ=0(inclusive),maxGQ=30(exclusive)\n##GVCFBlock30-100=minGQ=30(inclusive),maxGQ=100(exclusive)\n");
    same("no band", gvcf_header_lines({}), blocks + "##GVCFBlock0-100=minGQ=0(inclusive),maxGQ=100(exclusive)\n");
    same("#CHROM", vcf_chrom_line("NA1"), "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA1\n");
}

static PosLines lines_of(const char *tag, const std::vector<uint64_t> &pos) {
    PosLines l;
    for (uint64_t p : pos) l.begin_line(p) += tag + std::to_string(p) + "\n";
    return l;
}
static std::string positions(const PosLines &l) {
    std::string s;
    for (const auto &at : l.at) s += std::to_string(at.first) + "@" + std::to_string(at.second) + " ";
    return s;
}

static void test_merge() {
    PosLines out;
    merge_by_pos(lines_of("i", {5}), lines_of("s", {5}), true, out); // INDEL lines outer, SNV lines inner: the SNV line of a POS first
    same("SNV first", out.text, "s5\ni5\n");
    same("SNV first positions", positions(out), "5@0 5@3 ");
    merge_by_pos(lines_of("i", {5, 7}), lines_of("s", {3, 5, 9}), true, out);
    same("SNV and INDEL", out.text, "s3\ns5\ni5\ni7\ns9\n");
    same("positions", positions(out), "3@0 5@3 5@6 7@9 9@12 ");
    merge_by_pos(lines_of("b", {5}), lines_of("v", {5}), false, out); // block lines outer, VCF lines inner: the block's line first
    same("block first", out.text, "b5\nv5\n");
    merge_by_pos(lines_of("b", {1, 5, 9}), lines_of("v", {2, 5, 5, 8}), false, out);
    same("blocks and VCF", out.text, "b1\nv2\nb5\nv5\nv5\nv8\nb9\n");
    merge_by_pos(lines_of("b", {}), lines_of("v", {2, 5}), false, out);
    same("no outer", out.text, "v2\nv5\n");
    merge_by_pos(lines_of("b", {1, 5}), lines_of("v", {}), false, out);
    same("no inner", out.text, "b1\nb5\n");
    merge_by_pos(lines_of("b", {}), lines_of("v", {}), true, out);
    same("neither", out.text, "");
    same("neither positions", out.at.size(), 0);
    // an inner list that is not ascending keeps its order: a line waits behind the one in front of it
    merge_by_pos(lines_of("i", {4}), lines_of("s", {6, 2}), true, out);
    same("order kept", out.text, "i4\ns6\ns2\n");
}

static void test_callable_bed() {
    CallableBed bed;
    bed.add_block("chr1", 0, 7, DCN_BLOCK_REF + 1); // the last block of one stretch
    bed.add_block("chr1", 7, 5, DCN_BLOCK_REF + 3); // and the first of the next: another band, the same label
    bed.add_block("chr1", 13, 4, DCN_BLOCK_REF);    // behind a VARIANT position at 12, which is callable
    bed.add_block("chr1", 17, 3, DCN_BLOCK_NO_COVERAGE);
    bed.add_block("chr1", 20, 5, DCN_BLOCK_UNCALLED);
    same("nothing before it is known to be final", bed.rows, "chr1\t0\t17\tCALLABLE\nchr1\t17\t20\tNO_COVERAGE\n");
    bed.end_record("chr1", 30); // VARIANT positions to the record's end
    same("chr1", bed.rows, "chr1\t0\t17\tCALLABLE\nchr1\t17\t20\tNO_COVERAGE\nchr1\t20\t25\tLOW_CONFIDENCE\nchr1\t25\t30\tCALLABLE\n");
    bed.rows.clear();
    bed.add_block("chr2", 2, 6, DCN_BLOCK_NO_COVERAGE); // the cursor is at the new record's first base again
    bed.end_record("chr2", 8);
    same("chr2", bed.rows, "chr2\t0\t2\tCALLABLE\nchr2\t2\t8\tNO_COVERAGE\n");
    bed.rows.clear();
    bed.end_record("chr3", 4); // a record of VARIANT positions alone
    same("chr3", bed.rows, "chr3\t0\t4\tCALLABLE\n");
    bed.rows.clear();
    bed.add_block("chr4", 0, 4, DCN_BLOCK_REF); // CALLABLE at the end of chr3 and at the start of chr4 are two rows
    bed.end_record("chr4", 4);
    same("chr4", bed.rows, "chr4\t0\t4\tCALLABLE\n");
}

static void test_phase_sets() {
    const std::vector<std::string> names = {"chrA", "chrB"};
    const auto nothing = [](const char *what, const PhaseSets &got) {
        same(what, got.sets, 0), same(what, got.phased_sites, 0), same(what, got.links_joined, 0), same(what, got.n50, 0);
        same(what, got.set_rows, ""), same(what, got.link_rows, "");
    };
    nothing("no sites", phase_sets(nullptr, nullptr, 0, names));
    dcn_phase_site one = {};
    one.pos = 7;
    dcn_phase_result head = {};
    head.flags = DCN_PHASE_HEAD;
    nothing("one site", phase_sets(&one, &head, 1, names));
    // chrA: {100, 150, 220}, {500, 550}, 900 alone; chrB: {40, 100}
    const uint64_t pos[8] = {100, 150, 220, 500, 550, 900, 40, 100};
    const unsigned flags[8] = {DCN_PHASE_HEAD | DCN_PHASE_JOINED, DCN_PHASE_JOINED, 0, DCN_PHASE_HEAD | DCN_PHASE_JOINED, 0, DCN_PHASE_HEAD,
                               DCN_PHASE_HEAD | DCN_PHASE_JOINED, 0};
    dcn_phase_site sites[8] = {};
    dcn_phase_result res[8] = {};
    for (int s = 0; s < 8; ++s) {
        sites[s].pos = pos[s], sites[s].record = s < 6 ? 0 : 1;
        res[s].flags = (uint8_t)flags[s];
        res[s].link[0] = s, res[s].link[1] = 1, res[s].link[2] = 2, res[s].link[3] = 30 + s;
    }
    const PhaseSets got = phase_sets(sites, res, 8, names);
    same("sets", got.sets, 3), same("phased sites", got.phased_sites, 7), same("links joined", got.links_joined, 4);
    same("N50 of spans 121, 51, 61", got.n50, 121);
    same("set rows", got.set_rows, "chrA\t100\t220\t3\nchrA\t500\t550\t2\nchrB\t40\t100\t2\n");
    same("link rows", got.link_rows, "chrA\t100\t150\t0\t1\t2\t30\t1\nchrA\t150\t220\t1\t1\t2\t31\t1\nchrA\t220\t500\t2\t1\t2\t32\t0\n"
                                     "chrA\t500\t550\t3\t1\t2\t33\t1\nchrA\t550\t900\t4\t1\t2\t34\t0\nchrB\t40\t100\t6\t1\t2\t36\t1\n");
    same("phase sets header", phase_sets_header(), "record\tfirst_pos\tlast_pos\tsites\n");
    same("links header", links_header(), "record\tpos\tnext_pos\tn00\tn01\tn10\tn11\tjoined\n");
}

static void test_paf() {
    dcn_split_placement p = {};
    p.votes = 2, p.n_anchors = 7, p.n_positions = 9, p.read_start = 10, p.read_end = 110, p.ref_start = 1000, p.ref_end = 1100;
    p.rank = 0, p.n_placed = 1, p.rival_votes = 1, p.mapq = 60;
    const std::string front = "r1\t150\t10\t110\t+\tchr1\t5000\t1000\t1100\t", tags = "\t60\tcm:i:2\trk:i:0\tnp:i:1\trv:i:1\tna:i:7\tns:i:9";
    std::string s;
    append_paf(s, "r1", 150, p, "chr1", 5000, 31); // map: votes * k matches, at most the read's extent
    same("unverified", s, front + "62\t100" + tags + "\n");
    s.clear();
    append_paf(s, "r1", 150, p, "chr1", 5000, 31, DCN_VERIFY_OVER);
    same("over", s, front + "62\t100" + tags + "\tve:i:0\n");
    s.clear();
    append_paf(s, "r1", 150, p, "chr1", 5000, 31, 3);
    same("verified", s, front + "97\t100" + tags + "\tve:i:1\tNM:i:3\n");
    const uint32_t cigar[5] = {50u << 4 | DCN_CIGAR_EQUAL, 1u << 4 | DCN_CIGAR_DIFF, 2u << 4 | DCN_CIGAR_INS, 47u << 4 | DCN_CIGAR_EQUAL, 2u << 4 | DCN_CIGAR_DEL};
    s.clear();
    append_paf(s, "r1", 150, p, "chr1", 5000, 31, 5, cigar, 5);
    same("aligned", s, front + "97\t102" + tags + "\tve:i:1\tNM:i:5\tcg:Z:50=1X2I47=2D\n");
    s.clear();
    append_paf(s, "r1", 150, p, "chr1", 5000, 31, DCN_VERIFY_OVER, cigar, 0); // (a row over the limit has no runs)
    same("over, align", s, front + "62\t100" + tags + "\tve:i:0\n");
    s.clear();
    append_paf(s, "r1", 150, p, "chr1", 5000, 31, 0, cigar, 0);
    same("no runs", s, front + "0\t0" + tags + "\tve:i:1\tNM:i:0\tcg:Z:*\n");
    // extend: placed on [20, 100) of the read, carried to [5, 120) of its 150 bases; on a reverse row left and right swap
    dcn_split_placement placed = p, grown = p;
    placed.read_start = 20, placed.read_end = 100, grown.read_start = 5, grown.read_end = 120;
    same("extend tags forward", extend_tags(placed, grown, 150), "\txl:i:15\txr:i:20\tcl:i:5\tcr:i:30");
    placed.reverse = grown.reverse = 1;
    same("extend tags reverse", extend_tags(placed, grown, 150), "\txl:i:20\txr:i:15\tcl:i:30\tcr:i:5");
    s.clear();
    append_paf(s, "r1", 150, grown, "chr1", 5000, 31, 3, nullptr, 0, extend_tags(placed, grown, 150));
    same("reverse row with tags", s, "r1\t150\t5\t120\t-\tchr1\t5000\t1000\t1100\t112\t115" + tags + "\tve:i:1\tNM:i:3\txl:i:20\txr:i:15\tcl:i:30\tcr:i:5\n");
}

static void test_tables_and_params() {
    const uint32_t c[DCN_PILEUP_COLUMNS] = {1, 2, 3, 4, 5, 6, 7, 8}, qs[4] = {11, 20, 95, 40}, planes[4] = {0, 1, 2, 3};
    same("depth: A C G T N del", position_depth(c), 21);
    std::string s;
    append_pileup_row(s, "chr1", 12, 'A', c, nullptr, nullptr);
    same("pileup row", s, "chr1\t12\tA\t1\t2\t3\t4\t5\t6\t7\t8\n");
    s.clear();
    append_pileup_row(s, "chr1", 12, 'A', c, qs, planes);
    same("pileup row, call and strand", s, "chr1\t12\tA\t1\t2\t3\t4\t5\t6\t7\t8\t11\t20\t95\t40\t0\t1\t2\t3\n");
    same("pileup header", pileup_header(false, false), "record\tpos\tref\tA\tC\tG\tT\tN\tdel\tins\trev\n");
    same("pileup header, call", pileup_header(true, false), "record\tpos\tref\tA\tC\tG\tT\tN\tdel\tins\trev\tqA\tqC\tqG\tqT\n");
    same("pileup header, strand", pileup_header(true, true), "record\tpos\tref\tA\tC\tG\tT\tN\tdel\tins\trev\tqA\tqC\tqG\tqT\trA\trC\trG\trT\n");
    s.clear();
    append_site_row(s, "chr1", 12, 'A', 2u << 8 | 5u, 21);
    append_site_row(s, "chr1", 13, 'C', 4u << 8, 9);
    append_site_row(s, "chr1", 14, 'T', 9u << 8 | 1u, 2);
    same("site rows", s, "chr1\t12\tA\tG\t21\t5\nchr1\t13\tC\t-\t9\t0\nchr1\t14\tT\tN\t2\t1\n");
    dcn_insertion_allele al = {};
    al.len = 2, al.count = 6, al.events = 8;
    s.clear();
    append_insertion_variant(s, "chr1", 12, al, "GG", 21, false);
    al.flags = DCN_INSERTION_FRONT;
    append_insertion_variant(s, "chr1", 12, al, "GG", 21, true);
    same("insertion variants", s, "chr1\t12\tINS\t.\tGG\t21\t6\t8\nchr1\t12\tINS_FRONT\t.\tGG\t21\t6\t8\t.\t.\n");
    s.clear();
    append_call_variant(s, "chr1", 12, 'A', 'G', c, nullptr);
    append_call_variant(s, "chr1", 12, 'A', 'G', c, qs); // mean qualities 11 / 1 and 95 / 3, rounded down
    append_call_variant(s, "chr1", 12, 'A', '-', c, qs);
    append_call_variant(s, "chr1", 12, 'N', 'T', c, qs); // a record's base that is no column has no quality
    same("call variants", s, "chr1\t12\tSUB\tA\tG\t21\t3\t0\nchr1\t12\tSUB\tA\tG\t21\t3\t0\t11\t31\nchr1\t12\tDEL\tA\t-\t21\t6\t0\t.\t.\n"
                             "chr1\t12\tSUB\tN\tT\t21\t4\t0\t.\t10\n");
    dcn_split_placement p = {};
    p.read_start = 10, p.read_end = 110, p.ref_start = 1000, p.ref_end = 1100;
    s.clear();
    append_duplicate_row(s, "r1", 17, 3, "chr1", p); // rule D3: where the read's first base would lie, clipped bases included
    p.reverse = 1;
    append_duplicate_row(s, "r2", 18, 3, "chr1", p);
    p.reverse = 0, p.ref_start = 4;
    append_duplicate_row(s, "r3", 19, 0, "chr1", p);
    same("duplicate rows", s, "r1\t17\t3\tchr1\t+\t990\nr2\t18\t3\tchr1\t-\t1110\nr3\t19\t0\tchr1\t+\t-6\n");

    CallOptions o;
    o.ploidy = 1, o.min_depth = 4, o.min_frac = 600, o.min_gq = 21, o.min_qual = 22, o.indel_qual = 23, o.min_indel_count = 3;
    o.max_sb = 900, o.min_alt_strand = 2, o.min_strand_depth = 5, o.min_link_reads = 6, o.max_link_minor = 150, o.gq_bands = {10, 50};
    const dcn_genotype_params g = genotype_params(o);
    same("genotype params", std::to_string(g.ploidy) + " " + std::to_string(g.min_depth) + " " + std::to_string(g.min_gq) + " " + std::to_string(g.min_qual) + " " +
                            std::to_string(g.err_centi) + " " + std::to_string(g.het_centi), "1 4 21 22 477 301");
    const dcn_indel_params i = indel_params(o);
    same("indel params", std::to_string(i.ploidy) + " " + std::to_string(i.min_depth) + " " + std::to_string(i.min_gq) + " " + std::to_string(i.min_qual) + " " +
                         std::to_string(i.min_count) + " " + std::to_string(i.indel_centi) + " " + std::to_string(i.het_centi), "1 4 21 22 3 2300 301");
    const dcn_block_params b = block_params(o);
    same("block params", std::to_string(b.ploidy) + " " + std::to_string(b.min_depth) + " " + std::to_string(b.min_gq) + " " + std::to_string(b.min_qual) + " " +
                         std::to_string(b.err_centi) + " " + std::to_string(b.het_centi) + " " + std::to_string(b.n_edges) + " " + std::to_string(b.edges[0]) + " " +
                         std::to_string(b.edges[1]) + " " + std::to_string(b.edges[2]), "1 4 21 22 477 301 2 10 50 0");
    const dcn_strand_params st = strand_params(o);
    same("strand params", std::to_string(st.max_sb_centi) + " " + std::to_string(st.min_alt_strand) + " " + std::to_string(st.min_strand_depth), "900 2 5");
    const dcn_pileup_call_params pc = pileup_call_params(o);
    same("pileup call params", std::to_string(pc.min_depth) + " " + std::to_string(pc.min_permille), "4 600");
    const dcn_phase_params ph = phase_params(o);
    same("phase params", std::to_string(ph.min_reads) + " " + std::to_string(ph.max_minor_permille), "6 150");
}

int main() {
    test_genotype_alleles();
    test_snv_lines();
    test_indel_lines();
    test_block_lines();
    test_headers();
    test_merge();
    test_callable_bed();
    test_phase_sets();
    test_paf();
    test_tables_and_params();
    std::printf("%d checks bad %d\n", checks, bad);
    return bad != 0;
}
