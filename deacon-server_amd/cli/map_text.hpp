// map_text.hpp -- the text that the map family of the command-line tool writes (map, verify, align, pileup, extend, consensus,
// call, genotype, markdup, indels, normalize, strand, gvcf, phase), free of device calls: PAF lines, the pileup / sites /
// variants / duplicates / phase tables, the VCF header and its SNV, INDEL and block lines, the callable BED, the by-POS
// merge of two line lists, and the parameter structs of the calling modes from one options struct.  Every function appends
// to a std::string from plain inputs, so tests/cpp/map_text_test.cpp checks the text on a machine without a GPU.
// It depends on the three C headers and the standard library only, and calls no dcn_* function.
#pragma once
#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "deacon_hip.h"
#include "deacon_hip_blocks.h"
#include "deacon_hip_phase.h"

// one PAF line: the 12 columns, then cm (votes), rk (rank), np (placements of the read), rv (rival votes), na (anchor
// hits of the read), ns (positions of the read)
// (`verify`: edits = what dcn_verify_batch said of the row, and the line gains ve and, for a verified row, NM, with column
// 10 = column 11 - NM; map passes DCN_VERIFY_UNPLACED, which no placed row has, and prints what it always did)
// (`align`: cigar = the n_ops runs of a verified row, as dcn_align_batch gives them: column 10 = its '=' bases, column 11 =
// all its bases, and cg:Z: follows NM)
inline void append_paf(std::string &rows, const std::string &read_name, uint32_t read_len, const dcn_split_placement &p,
                       const std::string &record_name, uint32_t record_len, uint32_t k, uint32_t edits = DCN_VERIFY_UNPLACED,
                       const uint32_t *cigar = nullptr, uint64_t n_ops = 0, const std::string &more_tags = std::string()) {
    const uint64_t on_read = p.read_end - p.read_start, on_ref = p.ref_end - p.ref_start;
    const bool verified = edits != DCN_VERIFY_UNPLACED && edits != DCN_VERIFY_OVER;
    uint64_t matches = verified ? std::max(on_read, on_ref) - edits : std::min<uint64_t>((uint64_t)p.votes * k, on_read);
    uint64_t block = std::max(on_read, on_ref);
    if (verified && cigar) {
        matches = block = 0;
        for (uint64_t q = 0; q < n_ops; ++q) {
            block += cigar[q] >> 4;
            if ((cigar[q] & 15u) == DCN_CIGAR_EQUAL) matches += cigar[q] >> 4;
        }
    }
    rows.append(read_name);
    rows += '\t' + std::to_string(read_len) + '\t' + std::to_string(p.read_start) + '\t' + std::to_string(p.read_end) + '\t';
    rows += p.reverse ? '-' : '+';
    rows += '\t' + record_name + '\t' + std::to_string(record_len) + '\t' + std::to_string(p.ref_start) + '\t' +
            std::to_string(p.ref_end) + '\t' + std::to_string(matches) + '\t' + std::to_string(block) + '\t' +
            std::to_string(p.mapq);
    rows += "\tcm:i:" + std::to_string(p.votes) + "\trk:i:" + std::to_string(p.rank) + "\tnp:i:" + std::to_string(p.n_placed) +
            "\trv:i:" + std::to_string(p.rival_votes) + "\tna:i:" + std::to_string(p.n_anchors) + "\tns:i:" +
            std::to_string(p.n_positions);
    if (verified) rows += "\tve:i:1\tNM:i:" + std::to_string(edits);
    else if (edits == DCN_VERIFY_OVER) rows += "\tve:i:0";
    if (verified && cigar) {
        rows += "\tcg:Z:";
        for (uint64_t q = 0; q < n_ops; ++q) {
            const uint32_t op = cigar[q] & 15u;
            rows += std::to_string(cigar[q] >> 4);
            rows += op == DCN_CIGAR_EQUAL ? '=' : op == DCN_CIGAR_DIFF ? 'X' : op == DCN_CIGAR_INS ? 'I' : 'D';
        }
        if (n_ops == 0) rows += '*'; // (two empty extents: no placement call reports one)
    }
    rows += more_tags; // (`extend`: xl, xr, cl, cr)
    rows += '\n';
}

// (`extend`) the four tags of an extended row p that was `placed` before: what the flanks gave (xl, xr) and what is left
// of the read (cl, cr), in the record's direction
inline std::string extend_tags(const dcn_split_placement &placed, const dcn_split_placement &p, uint32_t read_len) {
    const uint64_t lo = placed.read_start - p.read_start, hi = p.read_end - placed.read_end;
    const uint64_t clip_lo = p.read_start, clip_hi = read_len - p.read_end;
    return "\txl:i:" + std::to_string(p.reverse ? hi : lo) + "\txr:i:" + std::to_string(p.reverse ? lo : hi) + "\tcl:i:" +
           std::to_string(p.reverse ? clip_hi : clip_lo) + "\tcr:i:" + std::to_string(p.reverse ? clip_lo : clip_hi);
}

// the genotype's alleles x <= y (G3's order: index y (y + 1) / 2 + x at ploidy 2; the index is the allele at ploidy 1)
struct GenotypeAlleles {
    unsigned x, y;
};
inline GenotypeAlleles genotype_alleles(unsigned gt, unsigned ploidy) {
    if (ploidy != 2) return {gt, gt};
    unsigned y = 0;
    while ((y + 1) * (y + 2) / 2 <= gt) ++y;
    return {gt - y * (y + 1) / 2, y};
}

// a position's depth: reads with a base, an N or a deletion there (P4: the columns up to DCN_PILEUP_DEL)
inline uint64_t position_depth(const uint32_t *c) {
    uint64_t depth = 0;
    for (int col = 0; col <= DCN_PILEUP_DEL; ++col) depth += c[col];
    return depth;
}

// ---- the parameter structs of the calling modes, from the options that the command line sets --------------------------------
struct CallOptions {
    unsigned ploidy = 2, min_depth = 3, min_frac = 500, min_gq = 20, min_qual = 20;
    unsigned indel_qual = 20, min_indel_count = 2;
    unsigned max_sb = 1083, min_alt_strand = 1, min_strand_depth = 3;
    unsigned min_link_reads = 2, max_link_minor = 200;
    std::vector<unsigned> gq_bands = {20, 40, 60, 80, 99};
};
// 1000 log10 3 and 1000 log10 2, rounded: rule G2's and G3's conventions
constexpr uint32_t ERR_CENTI = 477, HET_CENTI = 301;

inline dcn_pileup_call_params pileup_call_params(const CallOptions &o) {
    dcn_pileup_call_params p = {};
    p.min_depth = o.min_depth, p.min_permille = o.min_frac;
    return p;
}
inline dcn_genotype_params genotype_params(const CallOptions &o) {
    dcn_genotype_params p = {};
    p.ploidy = o.ploidy, p.min_depth = o.min_depth, p.min_gq = o.min_gq, p.min_qual = o.min_qual;
    p.err_centi = ERR_CENTI, p.het_centi = HET_CENTI;
    return p;
}
inline dcn_indel_params indel_params(const CallOptions &o) {
    dcn_indel_params p = {};
    p.ploidy = o.ploidy, p.min_depth = o.min_depth, p.min_gq = o.min_gq, p.min_qual = o.min_qual;
    p.min_count = o.min_indel_count, p.indel_centi = 100 * o.indel_qual, p.het_centi = HET_CENTI;
    return p;
}
inline dcn_strand_params strand_params(const CallOptions &o) {
    dcn_strand_params p = {};
    p.max_sb_centi = o.max_sb, p.min_alt_strand = o.min_alt_strand, p.min_strand_depth = o.min_strand_depth;
    return p;
}
inline dcn_block_params block_params(const CallOptions &o) { // (the bands are checked by the library)
    dcn_block_params p = {};
    p.ploidy = o.ploidy, p.min_depth = o.min_depth, p.min_gq = o.min_gq, p.min_qual = o.min_qual;
    p.err_centi = ERR_CENTI, p.het_centi = HET_CENTI;
    p.n_edges = (uint32_t)std::min<size_t>(o.gq_bands.size(), 16);
    for (size_t b = 0; b < o.gq_bands.size() && b < 16; ++b) p.edges[b] = (uint8_t)std::min(o.gq_bands[b], 255u);
    return p;
}
inline dcn_phase_params phase_params(const CallOptions &o) {
    dcn_phase_params p = {};
    p.min_reads = o.min_link_reads, p.max_minor_permille = o.max_link_minor;
    return p;
}

// ---- the tables ----------------------------------------------------------------------------------------------------------
// the pileup TSV: `call` adds the quality sums, `strand` the reverse planes
inline const char *pileup_header(bool call, bool strand) {
    return strand ? "record\tpos\tref\tA\tC\tG\tT\tN\tdel\tins\trev\tqA\tqC\tqG\tqT\trA\trC\trG\trT\n"
           : call ? "record\tpos\tref\tA\tC\tG\tT\tN\tdel\tins\trev\tqA\tqC\tqG\tqT\n"
                  : "record\tpos\tref\tA\tC\tG\tT\tN\tdel\tins\trev\n";
}
// c = the position's DCN_PILEUP_COLUMNS counters; qsums and planes = its four sums and planes, or nullptr
inline void append_pileup_row(std::string &rows, const std::string &record, uint64_t pos, char ref, const uint32_t *c,
                              const uint32_t *qsums, const uint32_t *planes) {
    rows += record + '\t' + std::to_string(pos) + '\t' + ref;
    for (int col = 0; col < DCN_PILEUP_COLUMNS; ++col) rows += '\t' + std::to_string(c[col]);
    for (int col = 0; qsums && col < 4; ++col) rows += '\t' + std::to_string(qsums[col]);
    for (int col = 0; planes && col < 4; ++col) rows += '\t' + std::to_string(planes[col]);
    rows += '\n';
}

inline const char *sites_header() { return "record\tpos\tref\tcall\tdepth\tflags\n"; }
// info = what dcn_anchor_map_pileup_call says of the site: the call's code in bits 8 .. 15, the flags below
inline void append_site_row(std::string &rows, const std::string &record, uint64_t pos, char ref, uint32_t info, uint64_t depth) {
    const uint32_t code = (info >> 8) & 0xFFu;
    rows += record + '\t' + std::to_string(pos) + '\t' + ref + '\t' + (code <= 4 ? "ACGT-"[code] : 'N') + '\t' + std::to_string(depth) + '\t' +
            std::to_string(info & 0xFFu) + '\n';
}

inline const char *variants_header(bool call) {
    return call ? "record\tpos\ttype\tref\talt\tdepth\tcount\tevents\tref_qual\talt_qual\n" : "record\tpos\ttype\tref\talt\tdepth\tcount\tevents\n";
}
inline int base_column(char ch) { return ch == 'A' ? DCN_PILEUP_A : ch == 'C' ? DCN_PILEUP_C : ch == 'G' ? DCN_PILEUP_G : ch == 'T' ? DCN_PILEUP_T : -1; }
// (`call`) the mean quality of a column's bases at a position, rounded down; "." when it has none
inline std::string mean_qual(const uint32_t *c, const uint32_t *qs, int col) {
    return col < 0 || c[col] == 0 ? std::string(".") : std::to_string(qs[col] / c[col]);
}
// a called insertion (rule L7): `call` leaves its two quality columns empty
inline void append_insertion_variant(std::string &rows, const std::string &record, uint64_t pos, const dcn_insertion_allele &al,
                                     const std::string &alt, uint64_t depth, bool call) {
    rows += record + '\t' + std::to_string(pos) + '\t' + (al.flags & DCN_INSERTION_FRONT ? "INS_FRONT" : "INS") + "\t.\t" + alt + '\t' +
            std::to_string(depth) + '\t' + std::to_string(al.count) + '\t' + std::to_string(al.events) + (call ? "\t.\t.\n" : "\n");
}
// a position whose call ('A' 'C' 'G' 'T' or '-') is not the record's base; qsums = the position's four sums (`call`) or nullptr
inline void append_call_variant(std::string &rows, const std::string &record, uint64_t pos, char ref, char call, const uint32_t *c,
                                const uint32_t *qsums) {
    const uint32_t best = call == '-' ? c[DCN_PILEUP_DEL] : c[call == 'A' ? DCN_PILEUP_A : call == 'C' ? DCN_PILEUP_C : call == 'G' ? DCN_PILEUP_G : DCN_PILEUP_T];
    rows += record + '\t' + std::to_string(pos) + '\t' + (call == '-' ? "DEL" : "SUB") + '\t' + ref + '\t' + call + '\t' +
            std::to_string(position_depth(c)) + '\t' + std::to_string(best) + "\t0";
    if (qsums && call == '-') rows += "\t.\t.";
    else if (qsums) rows += '\t' + mean_qual(c, qsums, base_column(ref)) + '\t' + mean_qual(c, qsums, base_column(call));
    rows += '\n';
}

inline const char *duplicates_header() { return "read\tordinal\tfirst\trecord\tstrand\tpos5\n"; }
// rule D3's end, from the read's first selected row p
inline void append_duplicate_row(std::string &rows, const std::string &read, uint64_t ordinal, uint64_t first, const std::string &record,
                                 const dcn_split_placement &p) {
    const long long pos5 = p.reverse ? (long long)(p.ref_end + p.read_start) : (long long)p.ref_start - (long long)p.read_start;
    rows += read + '\t' + std::to_string(ordinal) + '\t' + std::to_string(first) + '\t' + record + '\t' + (p.reverse ? '-' : '+') + '\t' +
            std::to_string(pos5) + '\n';
}

// ---- VCF -----------------------------------------------------------------------------------------------------------------
struct VcfModes { // which of the modes above `genotype` is on: each sets all in front of it
    bool indels = false, normalize = false, strand = false, phase = false;
};
// the header without its #CHROM line.  VCF 4.2, SNVs only: indels stay in --variants (`indels`: and as INDEL lines here)
inline std::string vcf_header(const std::string &version, const VcfModes &m, const std::vector<std::string> &names,
                              const std::vector<uint32_t> &lens) {
    std::string head = "##fileformat=VCFv4.2\n##source=deacon-hip " + version + "\n";
    for (size_t r = 0; r < names.size(); ++r) head += "##contig=<ID=" + names[r] + ",length=" + std::to_string(lens[r]) + ">\n";
    if (m.strand)
        head += "##FILTER=<ID=strand_bias,Description=\"SB at or above --max-sb: the allele and the strand are not independent\">\n"
                "##FILTER=<ID=one_strand,Description=\"Both strands cover the site, the allele is on fewer than --min-alt-strand reads of one\">\n";
    head += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth: reads with a base, an N or a deletion at the position\">\n";
    if (m.strand)
        head += "##INFO=<ID=SB,Number=1,Type=Float,Description=\"Strand bias: chi-square of the 2 x 2 table of allele by strand, one degree of freedom\">\n";
    if (m.indels)
        head += "##INFO=<ID=INDEL,Number=0,Type=Flag,Description=\"An insertion or a deletion\">\n"
                "##INFO=<ID=IDV,Number=1,Type=Integer,Description=\"Reads that carry the allele\">\n"
                "##INFO=<ID=IEV,Number=1,Type=Integer,Description=\"Insertions behind, or deletions that begin at, the position, of any allele\">\n";
    if (m.normalize) head += "##left_aligned=The positions of insertions and deletions are left-aligned per read\n";
    head += "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
            "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: phred gap to the second best genotype, at most 99\">\n"
            "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Bases A, C, G, T of at least the minimum base quality\">\n"
            "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Such bases per allele\">\n";
    if (m.strand)
        head += "##FORMAT=<ID=ADF,Number=R,Type=Integer,Description=\"AD on the forward strand\">\n"
                "##FORMAT=<ID=ADR,Number=R,Type=Integer,Description=\"AD on the reverse strand\">\n";
    head += "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods, at most 255\">\n";
    if (m.phase) head += "##FORMAT=<ID=PS,Number=1,Type=Integer,Description=\"Phase set: POS of the first site of the set the genotype is phased in\">\n";
    return head;
}
// (`gvcf`) what the block lines use, between the --vcf header and #CHROM: a band per GQ edge, and one below and one above
inline std::string gvcf_header_lines(const std::vector<unsigned> &gq_bands) {
    std::string head = "##ALT=<ID=NON_REF,Description=\"Any allele other than the reference's: the line is a reference block\">\n"
                       "##INFO=<ID=END,Number=1,Type=Integer,Description=\"Last position of the block\">\n"
                       "##FORMAT=<ID=MIN_DP,Number=1,Type=Integer,Description=\"Smallest DP of the block's positions\">\n";
    for (size_t b = 0; b <= gq_bands.size(); ++b) {
        const unsigned lo = b ? gq_bands[b - 1] : 0u, hi = b < gq_bands.size() ? gq_bands[b] : 100u;
        head += "##GVCFBlock" + std::to_string(lo) + "-" + std::to_string(hi) + "=minGQ=" + std::to_string(lo) + "(inclusive),maxGQ=" +
                std::to_string(hi) + "(exclusive)\n";
    }
    return head;
}
inline std::string vcf_chrom_line(const std::string &sample) { return "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample + "\n"; }

// the FILTER column and SB of a site's strand evidence
inline std::string strand_filter(const dcn_strand_site &e) {
    return e.flags == 0 ? "PASS" : e.flags == DCN_STRAND_BIAS ? "strand_bias" : e.flags == DCN_STRAND_ONE_SIDED ? "one_strand" : "strand_bias;one_strand";
}
inline std::string strand_sb(const dcn_strand_site &e) {
    char text[32];
    std::snprintf(text, sizeof text, "%u.%02u", e.sb_centi / 100u, e.sb_centi % 100u);
    return text;
}

// rule S3's query of an SNV site: ALT = the genotype's alleles other than the record's base
inline dcn_strand_query snv_strand_query(const dcn_genotype_site &g, unsigned ploidy) {
    const GenotypeAlleles al = genotype_alleles(g.gt, ploidy);
    dcn_strand_query q = {};
    q.pos = g.pos, q.ref_code = g.ref_code;
    q.alt_mask = ((1u << al.x) | (1u << al.y)) & ~(1u << g.ref_code);
    return q;
}

// (`phase`) the list entry of a heterozygous site: a0 the record's base when the genotype holds it, else the lower column
inline bool phase_site_of(const dcn_genotype_site &g, unsigned ploidy, uint32_t record, dcn_phase_site &site) {
    const GenotypeAlleles al = genotype_alleles(g.gt, ploidy);
    if (al.x == al.y) return false;
    site = dcn_phase_site{};
    site.pos = g.pos, site.record = record;
    site.a0 = (uint8_t)(al.y == g.ref_code ? al.y : al.x); // (x < y)
    site.a1 = (uint8_t)(al.y == g.ref_code ? al.x : al.y);
    return true;
}

// the line of an SNV site, written from the site alone: (REF, ALTs in A C G T order), PL in VCF's order over them.
//   st       the site's strand evidence (`strand`: FILTER, SB, ADF, ADR) or nullptr
//   ps, ph   (`phase`) the site's entry of the list and its result when the line is phased, else nullptr: g1|g2 and PS
inline void append_snv_line(std::string &rows, const std::string &record, const dcn_genotype_site &g, unsigned ploidy,
                            const dcn_strand_site *st = nullptr, const dcn_phase_site *ps = nullptr, const dcn_phase_result *ph = nullptr) {
    const GenotypeAlleles gt = genotype_alleles(g.gt, ploidy);
    const unsigned x = gt.x, y = gt.y;
    unsigned alleles[3] = {g.ref_code, 0, 0}, n_alleles = 1;
    if (x != g.ref_code) alleles[n_alleles++] = x;
    if (y != g.ref_code && y != x) alleles[n_alleles++] = y;
    const auto index_of = [&](unsigned c) { return c == alleles[0] ? 0u : c == alleles[1] ? 1u : 2u; };
    const auto pair_index = [](unsigned p, unsigned q) { return p <= q ? q * (q + 1) / 2 + p : p * (p + 1) / 2 + q; };
    rows += record + '\t' + std::to_string(g.pos + 1) + "\t.\t" + "ACGT"[g.ref_code] + '\t';
    for (unsigned k = 1; k < n_alleles; ++k) rows += std::string(k > 1 ? "," : "") + "ACGT"[alleles[k]];
    if (st)
        rows += '\t' + std::to_string(g.qual) + '\t' + strand_filter(*st) + "\tDP=" + std::to_string(g.depth) + ";SB=" + strand_sb(*st) +
                (ph ? "\tGT:GQ:DP:AD:ADF:ADR:PL:PS\t" : "\tGT:GQ:DP:AD:ADF:ADR:PL\t");
    else rows += '\t' + std::to_string(g.qual) + "\tPASS\tDP=" + std::to_string(g.depth) + "\tGT:GQ:DP:AD:PL\t";
    if (ph) { // haplotype 1 carries a[hap], haplotype 2 a[1 - hap] (rule H6)
        const unsigned al[2] = {ps->a0, ps->a1};
        rows += std::to_string(index_of(al[ph->hap & 1u])) + '|' + std::to_string(index_of(al[1u - (ph->hap & 1u)]));
    } else if (ploidy == 2) rows += std::to_string(std::min(index_of(x), index_of(y))) + '/' + std::to_string(std::max(index_of(x), index_of(y)));
    else rows += std::to_string(index_of(x));
    rows += ':' + std::to_string(g.gq) + ':' + std::to_string((uint64_t)g.ad[0] + g.ad[1] + g.ad[2] + g.ad[3]) + ':';
    for (unsigned k = 0; k < n_alleles; ++k) rows += (k ? "," : "") + std::to_string(g.ad[alleles[k]]);
    rows += ':';
    if (st) { // over the same alleles as AD
        for (unsigned k = 0; k < n_alleles; ++k) rows += (k ? "," : "") + std::to_string(st->fwd[alleles[k]]);
        rows += ':';
        for (unsigned k = 0; k < n_alleles; ++k) rows += (k ? "," : "") + std::to_string(st->rev[alleles[k]]);
        rows += ':';
    }
    bool first = true;
    for (unsigned j = 0; j < n_alleles; ++j)
        for (unsigned i = 0; i <= (ploidy == 2 ? j : 0u); ++i) {
            rows += (first ? "" : ",") + std::to_string(g.pl[ploidy == 2 ? pair_index(alleles[i], alleles[j]) : alleles[j]]);
            first = false;
        }
    if (ph) rows += ':' + std::to_string(ph->set_pos + 1);
    rows += '\n';
}

// bases [from, from + count) of a record of which text holds [start, start + n): the stretch's own, or what fetch(from,
// count) gives where a line reaches beyond it
template <typename Fetch>
std::string reference_bases(const uint8_t *text, uint64_t start, uint64_t n, uint64_t from, uint64_t count, Fetch fetch) {
    if (from >= start && from + count <= start + n) return std::string((const char *)text + (from - start), count);
    return fetch(from, count);
}

// POS, REF and ALT of an indel site (rules I6-I8): a deletion and an insertion in front take the base before them as the
// anchor, at the record's first position the base behind; ins = the bases array of the call that gave the site; ref_bases(from,
// count) gives the record's bases
struct IndelAlleles {
    uint64_t pos1;
    std::string ref, alt;
};
template <typename RefBases>
IndelAlleles indel_alleles(const dcn_indel_site &s, const uint8_t *ins_bases, RefBases ref_bases) {
    IndelAlleles v;
    if (s.flags & DCN_INDEL_DELETION) {
        v.ref = ref_bases(s.pos > 0 ? s.pos - 1 : 0, (uint64_t)s.len + 1);
        v.pos1 = s.pos > 0 ? s.pos : 1;
        v.alt = s.pos > 0 ? v.ref.substr(0, 1) : v.ref.substr(s.len, 1);
    } else {
        const std::string ins((const char *)ins_bases + s.bases_offset, s.len);
        const bool front = (s.flags & DCN_INDEL_FRONT) != 0;
        v.ref = ref_bases(front && s.pos > 0 ? s.pos - 1 : s.pos, 1);
        v.pos1 = front ? (s.pos > 0 ? s.pos : 1) : s.pos + 1;
        v.alt = front && s.pos == 0 ? ins + v.ref : v.ref + ins;
    }
    return v;
}
inline bool indel_is_hom(const dcn_indel_site &s, unsigned ploidy) { return s.gt == ploidy; } // V/V, or V at ploidy 1
// the INDEL line of a site; st = its strand evidence (`strand`) or nullptr
inline void append_indel_line(std::string &rows, const std::string &record, const IndelAlleles &v, const dcn_indel_site &s, unsigned ploidy,
                              const dcn_strand_site *st = nullptr) {
    const uint32_t others = s.depth >= s.count ? s.depth - s.count : 0;
    rows += record + '\t' + std::to_string(v.pos1) + "\t.\t" + v.ref + '\t' + v.alt + '\t' + std::to_string(s.qual) + '\t' +
            (st ? strand_filter(*st) : std::string("PASS")) + "\tINDEL;DP=" + std::to_string(s.depth) + ";IDV=" + std::to_string(s.count) +
            ";IEV=" + std::to_string(s.events) + (st ? ";SB=" + strand_sb(*st) + "\tGT:GQ:DP:AD:ADF:ADR:PL\t" : std::string("\tGT:GQ:DP:AD:PL\t")) +
            (ploidy == 1 ? "1" : indel_is_hom(s, ploidy) ? "1/1" : "0/1") + ':' + std::to_string(s.gq) + ':' +
            std::to_string((uint64_t)others + s.count) + ':' + std::to_string(others) + ',' + std::to_string(s.count) + ':';
    if (st) { // o,a split by strand: rule S4's table, a,c forward and b,d reverse
        const uint32_t *const t = st->table;
        rows += std::to_string(t[0]) + ',' + std::to_string(t[2]) + ':' + std::to_string(t[1]) + ',' + std::to_string(t[3]) + ':';
    }
    rows += std::to_string(s.pl[0]) + ',' + std::to_string(s.pl[1]);
    if (ploidy == 2) rows += ',' + std::to_string(s.pl[2]);
    rows += '\n';
}

// (`gvcf`) the line of a reference block; base = the record's base at its first position; DP is the mean depth rounded down
inline void append_block_line(std::string &rows, const std::string &record, const dcn_reference_block &b, uint8_t base, unsigned ploidy) {
    const bool is_ref = b.cls >= DCN_BLOCK_REF;
    rows += record + '\t' + std::to_string(b.pos + 1) + "\t.\t" + (char)std::toupper(base) + "\t<NON_REF>\t.\t.\tEND=" + std::to_string(b.pos + b.len) +
            "\tGT:GQ:DP:MIN_DP\t" + (is_ref ? (ploidy == 2 ? "0/0" : "0") : (ploidy == 2 ? "./." : ".")) + ':' + std::to_string(b.min_gq) + ':' +
            std::to_string(b.sum_depth / b.len) + ':' + std::to_string(b.min_depth) + '\n';
}

// ---- lines that carry their POS beside their text, and the merge of two such lists ---------------------------------------
struct PosLines {
    std::string text;
    std::vector<std::pair<uint64_t, size_t>> at; // per line: its POS and where it begins in text
    void clear() { text.clear(), at.clear(); }
    std::string &begin_line(uint64_t pos) { // the line is then appended to the string returned
        at.emplace_back(pos, text.size());
        return text;
    }
    size_t line_end(size_t i) const { return i + 1 < at.size() ? at[i + 1].second : text.size(); }
    void append_line_of(const PosLines &from, size_t i) { begin_line(from.at[i].first).append(from.text, from.at[i].second, from.line_end(i) - from.at[i].second); }
};
// out = the lines of `outer`, each behind the lines of `inner` not yet out whose POS is below its own, or equal to it when
// ties_inner_first; then the rest of `inner`.  Both orders are kept.  The INDEL lines of a stretch are outer to its SNV lines
// (the SNV line of a POS first), the block lines are outer to the VCF lines (a block's line in front of a VCF line of its POS).
inline void merge_by_pos(const PosLines &outer, const PosLines &inner, bool ties_inner_first, PosLines &out) {
    out.clear();
    size_t next = 0;
    for (size_t i = 0; i < outer.at.size(); ++i) {
        const uint64_t pos = outer.at[i].first;
        while (next < inner.at.size() && (inner.at[next].first < pos || (ties_inner_first && inner.at[next].first == pos))) out.append_line_of(inner, next++);
        out.append_line_of(outer, i);
    }
    while (next < inner.at.size()) out.append_line_of(inner, next++);
}

// ---- (`gvcf`) the callable BED: a record's final blocks in ascending order, neighbours of one label joined -------------------
struct CallableBed {
    std::string rows; // the caller writes and clears them
    // a final block [pos, pos + len) of class cls; the gap in front of it holds VARIANT positions, which are callable
    void add_block(const std::string &record, uint64_t pos, uint64_t len, uint32_t cls) {
        if (pos > cursor) add(record, cursor, pos, CALLABLE);
        add(record, pos, pos + len, cls == DCN_BLOCK_NO_COVERAGE ? NO_COVERAGE : cls >= DCN_BLOCK_REF ? CALLABLE : LOW_CONFIDENCE);
        cursor = pos + len;
    }
    void end_record(const std::string &record, uint64_t record_len) {
        if (record_len > cursor) add(record, cursor, record_len, CALLABLE);
        add(record, 0, 0, nullptr);
        cursor = 0;
    }

  private:
    static constexpr const char *NO_COVERAGE = "NO_COVERAGE", *LOW_CONFIDENCE = "LOW_CONFIDENCE", *CALLABLE = "CALLABLE";
    uint64_t from = 0, to = 0; // the interval that is open, [from, to) with label `label`
    const char *label = nullptr;
    uint64_t cursor = 0; // the first position of the record that no final block and no gap in front of one has covered
    void add(const std::string &record, uint64_t a, uint64_t b, const char *l) { // l = nullptr: the record ends
        if (l && label == l && to == a) {
            to = b;
            return;
        }
        if (label && to > from) rows += record + '\t' + std::to_string(from) + '\t' + std::to_string(to) + '\t' + label + '\n';
        from = a, to = b, label = l;
    }
};

// ---- (`phase`) the sets of a solved site list ------------------------------------------------------------------------------
inline const char *phase_sets_header() { return "record\tfirst_pos\tlast_pos\tsites\n"; }
inline const char *links_header() { return "record\tpos\tnext_pos\tn00\tn01\tn10\tn11\tjoined\n"; }
struct PhaseSets {
    uint64_t sets = 0, phased_sites = 0, links_joined = 0, n50 = 0; // sets of two sites or more (H7), and the N50 of their spans
    std::string set_rows, link_rows;
};
// sites and their results (dcn_anchor_map_phase_solve), n of each; names = the records' names
inline PhaseSets phase_sets(const dcn_phase_site *sites, const dcn_phase_result *res, size_t n, const std::vector<std::string> &names) {
    PhaseSets out;
    std::vector<uint64_t> spans;
    for (size_t s = 0; s < n;) {
        size_t e = s + 1; // the set [s, e)
        while (e < n && !(res[e].flags & DCN_PHASE_HEAD)) ++e;
        if (e - s >= 2) {
            ++out.sets, out.phased_sites += e - s;
            spans.push_back(sites[e - 1].pos - sites[s].pos + 1);
            out.set_rows += names[sites[s].record] + '\t' + std::to_string(sites[s].pos) + '\t' + std::to_string(sites[e - 1].pos) + '\t' +
                            std::to_string(e - s) + '\n';
        }
        s = e;
    }
    for (size_t s = 0; s + 1 < n; ++s) {
        out.links_joined += (res[s].flags & DCN_PHASE_JOINED) != 0;
        if (sites[s + 1].record != sites[s].record) continue;
        out.link_rows += names[sites[s].record] + '\t' + std::to_string(sites[s].pos) + '\t' + std::to_string(sites[s + 1].pos);
        for (int c = 0; c < 4; ++c) out.link_rows += '\t' + std::to_string(res[s].link[c]);
        out.link_rows += (res[s].flags & DCN_PHASE_JOINED) ? "\t1\n" : "\t0\n";
    }
    std::sort(spans.begin(), spans.end(), std::greater<uint64_t>());
    uint64_t total = 0, sum = 0;
    for (uint64_t v : spans) total += v;
    for (uint64_t v : spans) {
        sum += v;
        if (2 * sum >= total) {
            out.n50 = v;
            break;
        }
    }
    return out;
}
