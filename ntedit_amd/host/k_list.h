// k_list.h -- `ntedit --reads -k K1,K2,...,Kn`: the rules of a list of k and the {k} of the saved files' names.  Host only
// (main.cpp; the CPU tests compile it on its own).
#pragma once

#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

namespace nte_host {

// The rules of -k K1,K2,...,Kn, a cascade of polishing rounds: what is refused before the device is opened and before any
// file is written.  Returns the refusal, or "" and the k of the rounds as given, in order.
inline std::string
k_list_rules(const char* list, bool reads_mode, bool shard_given, bool have_prefix,
             const std::vector<std::pair<const char*, std::string>>& names, std::vector<std::string>* ks)
{
	const std::string k = std::string("-k ") + list;
	if (!reads_mode) {
		return k + ": a list of k polishes in a cascade of rounds, one filter built from the reads per k: only with --reads (not with -r or --genome)";
	}
	if (shard_given) {
		return k + " and --shard: a cascade of rounds runs on one device; the list of k is refused with --shard";
	}
	if (!have_prefix) {
		return k + ": a list of k needs -b (every round writes its files under the prefix: the last <prefix>_edited.fa, an earlier one "
		           "<prefix>_k<K>_edited.fa)";
	}
	std::vector<unsigned long> seen;
	const std::string text = list;
	for (size_t at = 0; at <= text.size();) {
		size_t comma = text.find(',', at);
		comma = comma == std::string::npos ? text.size() : comma;
		const std::string one = text.substr(at, comma - at);
		const bool digits = !one.empty() && one.size() <= 3 && one.find_first_not_of("0123456789") == std::string::npos;
		const unsigned long v = digits ? strtoul(one.c_str(), nullptr, 10) : 0;
		if (v < 12 || v > 200) {
			return k + ": k must be between 12 and 200 (`" + one + "')";
		}
		seen.push_back(v);
		ks->push_back(std::to_string(v));
		at = comma + 1;
	}
	if (seen.size() > 8) {
		return k + ": at most 8 k in a list (" + std::to_string(seen.size()) + " given)";
	}
	for (size_t i = 0; i < seen.size(); i++) {
		for (size_t j = 0; j < i; j++) {
			if (seen[i] == seen[j]) {
				return k + ": k = " + std::to_string(seen[i]) + " is given twice (a cascade polishes at each k once)";
			}
		}
	}
	for (const auto& n : names) {
		if (!n.second.empty() && n.second.find("{k}") == std::string::npos) {
			return std::string(n.first) + " " + n.second + ": with a list of k the name needs {k} (each round writes its own file, its k in place "
			                                               "of {k})";
		}
	}
	return "";
}

// `name` with every {k} replaced by k
inline std::string
with_k(std::string name, uint32_t k)
{
	const std::string kt = std::to_string(k);
	for (size_t at = 0; (at = name.find("{k}", at)) != std::string::npos; at += kt.size()) {
		name.replace(at, 3, kt);
	}
	return name;
}

} // namespace nte_host
