// segclust_host.cpp -- the host side of the segment clustering (include/amx.h, section "segment clustering"): the defaults of the node's
// parameters, the BIC choice over the tracker records with the class ids it implies (findBestBIC and returnClustering,
// Signal/SegmentClustering.hh:775-814), and the key-map file (printClustering, :754-772).  No device.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "common.hpp"

extern "C" {

void amx_segclust_default_cfg(amx_segclust_cfg* cfg) {
    if (!cfg)
        return;
    *cfg            = amx_segclust_cfg{};
    cfg->minframes  = 0;
    cfg->mincluster = 2;
    cfg->maxcluster = 100000;
    cfg->threshold  = 0.f;
    cfg->lambda     = 1.f;
    cfg->alpha      = -1.f;   // automatic
    cfg->minalpha   = 0.40f;
    cfg->maxalpha   = 0.60f;
    cfg->amalgamation = 0;
    cfg->infile       = nullptr;
}

int amx_segclust_choose(int n, const int32_t* parent, const int32_t* child, const float* score, int mincluster, int maxcluster, int32_t* class_ids,
                        int* n_clusters, int* best_index) {
    const char* who = "amx_segclust_choose";
    AMX_REQUIRE(n >= 1 && class_ids, AMX_ERR_INVALID, "%s: n %d or NULL class_ids", who, n);
    AMX_REQUIRE(n == 1 || (parent && child && score), AMX_ERR_INVALID, "%s: NULL tracker list", who);
    // mincluster 0 lets the reference read one record past its tracker list, maxcluster 0 starts it there
    AMX_REQUIRE(mincluster >= 1 && maxcluster >= 1, AMX_ERR_INVALID, "%s: mincluster %d, maxcluster %d: both must be at least 1", who, mincluster, maxcluster);
    AMX_REQUIRE(mincluster <= n, AMX_ERR_UNSUPPORTED, "%s: mincluster %d is larger than the %d segments (the reference's unsigned difference wraps)", who,
                mincluster, n);
    std::vector<char> seen(n, 0);
    for (int i = 0; i < n - 1; ++i) {
        AMX_REQUIRE(parent[i] >= 0 && parent[i] < child[i] && child[i] < n && !seen[child[i]] && !seen[parent[i]], AMX_ERR_INVALID,
                    "%s: record %d merges %d into %d: not a pair of live clusters with parent < child", who, i, child[i], parent[i]);
        seen[child[i]] = 1;
    }
    // findBestBIC: the cumulative score's strict minimum below 0, from the first record maxcluster leaves open up to the last mincluster allows
    int       best = -1;
    float     best_score = 0.f, current = 0.f;
    const int stop = n - mincluster;
    if (n > maxcluster)
        best = n - maxcluster - 1;
    for (int i = best + 1; i < stop; ++i) {
        current += score[i];
        if (current < best_score)
            best_score = current, best = i;
    }
    // returnClustering: replay the records up to the chosen one, then follow every slot to its live root
    std::vector<char> live(n, 1);
    for (int i = 0; i < n; ++i)
        class_ids[i] = i;
    for (int i = 0; i <= best; ++i) {
        live[child[i]]      = 0;
        class_ids[child[i]] = parent[i];
    }
    int clusters = live[0] ? 1 : 0;
    for (int i = n - 1; i > 0; --i) {
        int j = i;
        while (!live[j])
            j = class_ids[j];
        class_ids[i] = j;
        clusters += live[i] ? 1 : 0;
    }
    if (n_clusters)
        *n_clusters = clusters;
    if (best_index)
        *best_index = best;
    return AMX_OK;
}

// putEscaped(value, "&<>\"'") of Core::XmlWriter::putTag
static std::string xml_escaped(const char* s) {
    std::string out;
    for (; *s; ++s)
        switch (*s) {
        case '&': out += "&amp;"; break;
        case '<': out += "&lt;"; break;
        case '>': out += "&gt;"; break;
        case '"': out += "&quot;"; break;
        case '\'': out += "&apos;"; break;
        default: out += *s;
        }
    return out;
}

// printClustering on a Core::XmlOutputStream, the writer amx_cmllr_transform_write restates: the declaration the stream puts in front, the
// element `coprus-key-map` (sic), one empty element per line (the stream neither indents nor wraps by default), the default cluster's keys first
// with value 0.  class_ids are written as given: amx_segclust_cluster has already moved them up by one where a default cluster exists.
int amx_segclust_write_map(const char* path, const char* const* ids, int n_default, const char* const* default_ids, int n, const int32_t* class_ids) {
    const char* who = "amx_segclust_write_map";
    AMX_REQUIRE(path && n >= 0 && n_default >= 0 && (n == 0 || (ids && class_ids)) && (n_default == 0 || default_ids), AMX_ERR_INVALID,
                "%s: NULL argument or negative count", who);
    for (int i = 0; i < n; ++i)
        AMX_REQUIRE(ids[i] && class_ids[i] >= 0, AMX_ERR_INVALID, "%s: segment %d has no id or a negative class", who, i);
    for (int i = 0; i < n_default; ++i)
        AMX_REQUIRE(default_ids[i], AMX_ERR_INVALID, "%s: default segment %d has no id", who, i);
    FILE* f = fopen(path, "wb");
    AMX_REQUIRE(f, AMX_ERR_INVALID, "%s: cannot open '%s'", who, path);
    bool ok = fputs("<?xml version=\"1.0\" encoding=\"ISO-8859-1\"?>\n<coprus-key-map>\n", f) >= 0;
    for (int i = 0; ok && i < n_default; ++i)
        ok = fprintf(f, "<map-item key=\"%s\" value=\"0\"/>\n", xml_escaped(default_ids[i]).c_str()) > 0;
    for (int i = 0; ok && i < n; ++i)
        ok = fprintf(f, "<map-item key=\"%s\" value=\"%d\"/>\n", xml_escaped(ids[i]).c_str(), (int)class_ids[i]) > 0;
    ok = ok && fputs("</coprus-key-map>\n", f) >= 0;
    ok = (fclose(f) == 0) && ok;
    AMX_REQUIRE(ok, AMX_ERR_INVALID, "%s: write to '%s' failed", who, path);
    return AMX_OK;
}

}  // extern "C"
