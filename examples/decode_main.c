/*
 * decode_main.c -- the reference driver (paged_infer.c:953-1101) on the
 * MI355X decode path, written against the drop-in C API only:
 *
 *   build the model (checkpoint, :436-502; or seeded synthetic GPT-2 124M)
 *   -> hand it a caller-owned BlockManager (:986-987)
 *   -> read the prompt tokens (the reference's DataLoader reads int32
 *      tokens, :753-818; synthetic ids when no file is given)
 *   -> prefill every prompt in one pass (gpt2_decode_prefill: B*T-row GEMMs,
 *      causal multi-query paged attention on MFMA)
 *   -> decode: sample_mult with random_f32 coins from xorshift state 1337
 *      (:1060-1062; on the device, sequence b seeded 1337 + b) or greedy
 *   -> print every token through the tokenizer (:875-928; ids when there is
 *      no tokenizer file), time the generation (:1019-1020, :1085-1087).
 *
 *   gcc -O2 examples/decode_main.c -Iinclude -Lllm.c-paged_amd -lpaged_hip \
 *       -Wl,-rpath,$PWD/llm.c-paged_amd -o decode_main
 *   ./decode_main [-c checkpoint.bin] [-k tokenizer.bin] [-t tokens.bin]
 *                 [-b B] [-p prompt_len] [-n new_tokens] [-g] [-o ids.bin] [-q]
 *                 [--temperature X] [--top-k N] [--top-p X] [--perplexity] [--logprobs]
 *                 [--speculate K] [--speculate-sampled K] [--repetition-penalty R] [--presence-penalty X]
 *                 [--frequency-penalty X] [--ban ID]... [--top-logprobs K]
 *                 [--speculate-tree N] [--tree-depth D] [--tree-branches W] [--speculate-tree-sampled N]
 *                 [--park-at N]
 *     -g greedy (default: sampling as the reference), -o writes the B x
 *     (prompt + new) token ids as int32, -q prints only the summary line.
 *     --temperature / --top-k / --top-p: any of them selects filtered
 *     sampling (gpt2_decode_set_sampling mode 2) with these settings for
 *     every sequence (defaults 1, 0 = off, 1 = off); -g still wins.
 *     --perplexity: the prompt pass is gpt2_decode_score with shifted targets
 *     (token t+1 scores position t): prints the mean negative log-likelihood
 *     and its exp per sequence and overall.  --logprobs: prints sequence 0's
 *     log-probability beside each generated token (gpt2_decode_set_logprobs:
 *     the raw model distribution, whatever the sampling settings).
 *     --speculate-sampled K (1..7, without -g): the same loop under filtered
 *     sampling (mode 2, with --temperature / --top-k / --top-p or their
 *     defaults): gpt2_decode_verify_sampled accepts a draft with the
 *     probability the sampler gives it and resamples at the first rejection;
 *     the emitted tokens are distributed as token-by-token sampling.
 *     --speculate K (1..7, with -g only): speculative greedy decoding.  Every
 *     pass drafts up to K tokens per sequence with the n-gram drafter
 *     (gpt2_ngram_draft over prompt + output, n-grams of 3 down to 1 tokens)
 *     and verifies them in one gpt2_decode_verify pass, which emits the
 *     accepted drafts and one token of the model's own.  The ids are those of
 *     plain greedy decoding; one more line reports passes, tokens and the mean
 *     number of accepted drafts per sequence and pass.  Not with --logprobs.
 *     --speculate-tree N (1..7 nodes, with -g only; --tree-depth D, default 4;
 *     --tree-branches W, default 3): the same loop over draft TREES.  Every
 *     pass merges the continuations of up to W earlier occurrences of the
 *     suffix into a tree of at most N drafts, D deep (gpt2_ngram_draft_tree),
 *     and gpt2_decode_verify_tree verifies every branch in one pass.  The ids
 *     are those of plain greedy decoding; the closing line also reports how
 *     many (sequence, pass) pairs continued from a node that was not on the
 *     tree's first branch (what a chain draft would have lost).  Exclusive with
 *     --speculate, --speculate-sampled, sampling and processor flags.
 *     --speculate-tree-sampled N (1..7 nodes, without -g; with --tree-depth,
 *     --tree-branches, --temperature, --top-k, --top-p): the tree loop under
 *     filtered sampling (mode 2).  gpt2_decode_verify_tree_sampled examines the
 *     children of a node in turn, each against what the siblings rejected
 *     before it left of the node's distribution, and draws the sequence's own
 *     token from the rest: the emitted tokens are distributed as token-by-token
 *     sampling.  Reports the passes that continued off the first branch like
 *     --speculate-tree.  Not with -g, the other --speculate flags or the
 *     penalty flags.
 *     --repetition-penalty R (> 0, 1 = off; the HF rule), --presence-penalty X,
 *     --frequency-penalty X (0 = off; the OpenAI rule) and --ban ID (repeatable,
 *     up to HPA_LOGIT_BIAS_MAX ids that are never produced): any of them turns
 *     the logit processors on (gpt2_decode_set_processors) with these settings
 *     for every sequence.  The window starts at position 0, so the prompt's
 *     tokens count.  They apply in every mode, -g included (GPT-2 124M loops
 *     within a few dozen greedy tokens without them).  Not with --speculate.
 *     --top-logprobs K (1..HPA_TOP_LOGPROBS_MAX): prints sequence 0's K most
 *     likely ids with their log-probabilities beside each generated token
 *     (gpt2_decode_set_top_logprobs: the raw model distribution, whatever the
 *     sampling settings and processors); with --perplexity the prompt pass is
 *     gpt2_decode_score_top and every prompt position of sequence 0 prints its
 *     K alternatives.  Not with --speculate.
 *     --park-at N (1 <= N < new_tokens): after N generated tokens every sequence
 *     is parked (gpt2_decode_park: its K/V pages and everything else that
 *     belongs to it into host memory), the pool is shown empty
 *     (gpt2_decode_free_pages), and sequence b is unparked into slot (b + 1) % B
 *     (gpt2_decode_unpark), where it continues as if it had never left: the
 *     text and the ids are those of the run without the flag, sampled runs
 *     included (the sampler state travels).  Not with --speculate.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "block_manager.h"
#include "hip_paged_attn.h"
#include "paged_infer.h"

static double now_s(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec + 1e-9 * t.tv_nsec;
}

/* e^x without libm (this file links against libpaged_hip only): halve the
 * argument into [-0.5, 0.5], Taylor series, square back */
static double exp_d(double x) {
    int n = 0;
    while (x > 0.5 || x < -0.5) { x *= 0.5; n++; }
    double s = 1.0, term = 1.0;
    for (int i = 1; i < 20; i++) { term *= x / i; s += term; }
    while (n--) s *= s;
    return s;
}

static void print_token(Tokenizer* tk, int id) {
    if (tk->init_ok) safe_printf(tokenizer_decode(tk, (unsigned)id));
    else printf("%d ", id);
}

/* " {id or text: logprob, ...}": the k alternatives of one row, most likely first */
static void print_alternatives(Tokenizer* tk, const int* ids, const float* lps, int k) {
    printf(" {");
    for (int j = 0; j < k; j++) {
        if (j) printf(", ");
        if (tk->init_ok) { printf("'"); safe_printf(tokenizer_decode(tk, (unsigned)ids[j])); printf("'"); }
        else printf("%d", ids[j]);
        printf(": %.4f", lps[j]);
    }
    printf("}");
}

int main(int argc, char** argv) {
    const char *ckpt = NULL, *tok_path = NULL, *tokens_path = NULL, *ids_out = NULL;
    int B = 4, prompt_len = 32, new_tokens = 32, greedy = 0, quiet = 0, filtered = 0, top_k = 0;
    int perplexity = 0, logprobs = 0, speculate = 0, spec_sampled = 0, top_lp = 0;
    int spec_tree = 0, spec_chain = 0, tree_depth = 4, tree_branches = 3, tree_flags = 0, park_on = 0, park_at = 0;
    float temperature = 1.0f, top_p = 1.0f;
    int processors = 0, n_ban = 0, ban[HPA_LOGIT_BIAS_MAX];
    float repetition = 1.0f, presence = 0.0f, frequency = 0.0f, ban_value[HPA_LOGIT_BIAS_MAX];
    for (int i = 1; i < argc; i++) {
        const char* a = argv[i];
        const char* v = i + 1 < argc ? argv[i + 1] : NULL;
        if (!strcmp(a, "-g")) { greedy = 1; continue; }
        if (!strcmp(a, "-q")) { quiet = 1; continue; }
        if (!strcmp(a, "--perplexity")) { perplexity = 1; continue; }
        if (!strcmp(a, "--logprobs")) { logprobs = 1; continue; }
        if (!v) { fprintf(stderr, "missing value for %s\n", a); return 2; }
        if (!strcmp(a, "-c")) ckpt = v;
        else if (!strcmp(a, "-k")) tok_path = v;
        else if (!strcmp(a, "-t")) tokens_path = v;
        else if (!strcmp(a, "-o")) ids_out = v;
        else if (!strcmp(a, "-b")) B = atoi(v);
        else if (!strcmp(a, "-p")) prompt_len = atoi(v);
        else if (!strcmp(a, "-n")) new_tokens = atoi(v);
        else if (!strcmp(a, "--temperature")) { temperature = (float)atof(v); filtered = 1; }
        else if (!strcmp(a, "--top-k")) { top_k = atoi(v); filtered = 1; }
        else if (!strcmp(a, "--top-p")) { top_p = (float)atof(v); filtered = 1; }
        else if (!strcmp(a, "--speculate")) { speculate = atoi(v); spec_chain = 1; }
        else if (!strcmp(a, "--speculate-sampled")) { speculate = atoi(v); spec_chain = spec_sampled = filtered = 1; }
        else if (!strcmp(a, "--speculate-tree")) { speculate = atoi(v); spec_tree = 1; tree_flags++; }
        else if (!strcmp(a, "--speculate-tree-sampled")) {
            speculate = atoi(v);
            spec_tree = spec_sampled = filtered = 1;
            tree_flags += 2;
        }
        else if (!strcmp(a, "--park-at")) { park_at = atoi(v); park_on = 1; }
        else if (!strcmp(a, "--tree-depth")) tree_depth = atoi(v);
        else if (!strcmp(a, "--tree-branches")) tree_branches = atoi(v);
        else if (!strcmp(a, "--top-logprobs")) {
            top_lp = atoi(v);
            if (top_lp < 1 || top_lp > HPA_TOP_LOGPROBS_MAX) {
                fprintf(stderr, "--top-logprobs takes 1..%d\n", HPA_TOP_LOGPROBS_MAX);
                return 2;
            }
        }
        else if (!strcmp(a, "--repetition-penalty")) { repetition = (float)atof(v); processors = 1; }
        else if (!strcmp(a, "--presence-penalty")) { presence = (float)atof(v); processors = 1; }
        else if (!strcmp(a, "--frequency-penalty")) { frequency = (float)atof(v); processors = 1; }
        else if (!strcmp(a, "--ban")) {
            if (n_ban >= HPA_LOGIT_BIAS_MAX) { fprintf(stderr, "at most %d --ban ids\n", HPA_LOGIT_BIAS_MAX); return 2; }
            ban[n_ban] = atoi(v);
            ban_value[n_ban++] = -1.0f / 0.0f; /* -inf: a hard ban */
            processors = 1;
        }
        else { fprintf(stderr, "unknown option %s\n", a); return 2; }
        i++;
    }
    if (spec_tree && (spec_chain || tree_flags > 2 || speculate < 1 || speculate > HPA_VERIFY_MAX_ROWS - 1 || tree_depth < 1 ||
                      tree_branches < 1)) {
        fprintf(stderr, "--speculate-tree and --speculate-tree-sampled take 1..%d nodes (--tree-depth and --tree-branches "
                        ">= 1) and go with no other --speculate flag\n", HPA_VERIFY_MAX_ROWS - 1);
        return 2;
    }
    if (speculate) {
        if (speculate < 1 || speculate > HPA_VERIFY_MAX_ROWS - 1) {
            fprintf(stderr, "--speculate takes 1..%d drafts\n", HPA_VERIFY_MAX_ROWS - 1);
            return 2;
        }
        if (spec_sampled && greedy) {
            fprintf(stderr, "--speculate-sampled and --speculate-tree-sampled sample (mode 2): not with -g (--speculate and "
                            "--speculate-tree are the greedy passes)\n");
            return 2;
        }
        if (!spec_sampled && (!greedy || filtered || logprobs || top_lp)) {
            fprintf(stderr, "--speculate is greedy only: give -g, and none of --temperature, --top-k, --top-p, "
                            "--logprobs, --top-logprobs\n");
            return 2;
        }
        if (processors) {
            fprintf(stderr, "--speculate does not go with --repetition-penalty, --presence-penalty, "
                            "--frequency-penalty or --ban: a verify pass has no per-row counts\n");
            return 2;
        }
    }
    if (park_on && (speculate || park_at < 1 || park_at >= new_tokens)) {
        fprintf(stderr, "--park-at takes 1..new_tokens - 1 and does not go with the --speculate flags\n");
        return 2;
    }
    GPT2 model;
    if (ckpt) {
        gpt2_build_from_checkpoint(&model, ckpt); /* exits on error, as the reference */
    } else {
        GPT2Config c = {1024, 50257, 12, 12, 768};
        if (gpt2_build_synthetic(&model, c, 1337ULL)) return 1;
    }
    const int V = model.config.vocab_size, total = prompt_len + new_tokens;
    if (B <= 0 || prompt_len <= 0 || new_tokens < 0 || total > model.config.max_seq_len) {
        fprintf(stderr, "need B > 0, prompt > 0 and prompt + new <= %d\n", model.config.max_seq_len);
        return 2;
    }
    const int page_size = 16, max_pages = (total + page_size - 1) / page_size;
    /* the caller owns the manager and hands it to the model (paged_infer.c:986-987) */
    BlockManager* bm = create_block_manager_ex(model.config.channels, B, B * max_pages, page_size, max_pages);
    if (!bm) return 1;
    model.manager = bm;
    if (gpt2_decode_init(&model, B, page_size, total)) return 1;
    if (!greedy && gpt2_decode_set_sampling(&model, filtered ? 2 : 1, 1337ULL)) return 1; /* rng_state = 1337 (:975) */
    if (!greedy && filtered && gpt2_decode_set_sampling_params(&model, -1, temperature, top_k, top_p)) return 2;
    if (logprobs && gpt2_decode_set_logprobs(&model, 1)) return 1;
    if (top_lp && gpt2_decode_set_top_logprobs(&model, top_lp)) return 1;
    if (processors) { /* bad values are refused with a message by the setters */
        if (gpt2_decode_set_processors(&model, 1)) return 1;
        if (gpt2_decode_set_penalties(&model, -1, repetition, presence, frequency, 0)) return 2;
        if (gpt2_decode_set_logit_bias(&model, -1, ban, ban_value, n_ban)) return 2;
    }
    gpt2_decode_set_graph(&model, 1);

    int* gen = (int*)malloc((size_t)B * total * sizeof(int));
    int* prompt = (int*)malloc((size_t)B * prompt_len * sizeof(int));
    int* next = (int*)malloc(B * sizeof(int));
    float* lp = (float*)malloc(B * sizeof(float));
    int* alt_ids = (int*)malloc((size_t)B * HPA_TOP_LOGPROBS_MAX * sizeof(int));
    float* alt_lps = (float*)malloc((size_t)B * HPA_TOP_LOGPROBS_MAX * sizeof(float));
    if (!gen || !prompt || !next || !lp || !alt_ids || !alt_lps) return 1;
    if (tokens_path) { /* int32 tokens, e.g. a prepro_tinyshakespeare.py .bin */
        FILE* f = fopen(tokens_path, "rb");
        if (!f || fread(prompt, sizeof(int), (size_t)B * prompt_len, f) != (size_t)B * prompt_len) {
            fprintf(stderr, "cannot read %d x %d tokens from %s\n", B, prompt_len, tokens_path);
            return 1;
        }
        fclose(f);
    } else {
        unsigned long long rng = 42;
        for (int i = 0; i < B * prompt_len; i++) prompt[i] = (int)(random_u32(&rng) % (unsigned)V);
    }
    for (int i = 0; i < B * prompt_len; i++)
        if (prompt[i] < 0 || prompt[i] >= V) { fprintf(stderr, "prompt token out of range\n"); return 1; }
    Tokenizer tk;
    tk.init_ok = 0;
    if (tok_path) tokenizer_init(&tk, tok_path);

    if (!quiet) {
        printf("==============Prompt (sequence 0):==================\n");
        for (int t = 0; t < prompt_len; t++) print_token(&tk, prompt[t]);
        printf("\n========================================\n");
    }
    double t0 = now_s();
    /* the whole prompt of every sequence in one pass; next[b] = the first new token */
    if (perplexity) { /* the same pass, scoring every prompt token against its successor */
        const size_t R = (size_t)B * prompt_len;
        int* lens = (int*)malloc(B * sizeof(int));
        int* targets = (int*)malloc(R * sizeof(int));
        float* score = (float*)malloc(R * sizeof(float));
        if (!lens || !targets || !score) return 1;
        for (int b = 0; b < B; b++) {
            lens[b] = prompt_len;
            for (int t = 0; t < prompt_len; t++)
                targets[(size_t)b * prompt_len + t] = t + 1 < prompt_len ? prompt[(size_t)b * prompt_len + t + 1] : -1;
        }
        if (top_lp) { /* the dense route: every prompt row's alternatives too */
            int* row_ids = (int*)malloc(R * top_lp * sizeof(int));
            float* row_lps = (float*)malloc(R * top_lp * sizeof(float));
            if (!row_ids || !row_lps) return 1;
            if (gpt2_decode_score_top(&model, prompt, lens, targets, score, top_lp, row_ids, row_lps, next)) return 1;
            for (int t = 0; t < prompt_len && !quiet; t++) { /* sequence 0's rows come first */
                printf("position %d after ", t);
                print_token(&tk, prompt[t]);
                printf(":");
                print_alternatives(&tk, row_ids + (size_t)t * top_lp, row_lps + (size_t)t * top_lp, top_lp);
                printf("\n");
            }
            free(row_ids);
            free(row_lps);
        } else if (gpt2_decode_score(&model, prompt, lens, targets, score, NULL, next)) {
            return 1;
        }
        double all = 0.0;
        for (int b = 0; b < B && prompt_len > 1; b++) {
            double nll = 0.0;
            for (int t = 0; t + 1 < prompt_len; t++) nll -= score[(size_t)b * prompt_len + t];
            all += nll;
            nll /= prompt_len - 1;
            printf("sequence %d: mean NLL %.6f, perplexity %.4f over %d tokens\n", b, nll, exp_d(nll), prompt_len - 1);
        }
        if (prompt_len > 1) {
            all /= (double)B * (prompt_len - 1);
            printf("overall: mean NLL %.6f, perplexity %.4f over %d tokens\n", all, exp_d(all), B * (prompt_len - 1));
        }
        free(lens);
        free(targets);
        free(score);
    } else if (gpt2_decode_prefill(&model, prompt, prompt_len, next)) {
        return 1;
    }
    double t1 = now_s();
    if (logprobs && gpt2_decode_logprobs(&model, lp)) return 1;
    if (top_lp && gpt2_decode_top_logprobs(&model, alt_ids, alt_lps)) return 1;
    for (int b = 0; b < B; b++) {
        memcpy(gen + (size_t)b * total, prompt + (size_t)b * prompt_len, prompt_len * sizeof(int));
        if (new_tokens > 0) gen[(size_t)b * total + prompt_len] = next[b];
    }
    if (!quiet) printf("\ngenerating:\n---\n");
    long spec_passes = 0, spec_live = 0, spec_accepted = 0, spec_tokens = 0, spec_off_first = 0;
    if (speculate && new_tokens > 0) {
        /* count[b] tokens of sequence b are out (the prefill's pick is the first and is b's pending id) */
        int* count = (int*)malloc(B * sizeof(int));
        int* n_draft = (int*)malloc(B * sizeof(int));
        int* n_acc = (int*)malloc(B * sizeof(int));
        int* drafts = (int*)malloc((size_t)B * HPA_VERIFY_MAX_ROWS * sizeof(int));
        int* out = (int*)malloc((size_t)B * HPA_VERIFY_MAX_ROWS * sizeof(int));
        int* parents = (int*)malloc((size_t)B * HPA_VERIFY_MAX_ROWS * sizeof(int));
        int* nodes = (int*)malloc((size_t)B * HPA_VERIFY_MAX_ROWS * sizeof(int));
        int* d0 = (int*)malloc(B * sizeof(int));
        if (!count || !n_draft || !n_acc || !drafts || !out || !parents || !nodes || !d0) return 1;
        for (int b = 0; b < B; b++) count[b] = 1;
        if (!quiet) print_token(&tk, next[0]);
        for (;;) {
            int live = 0, nd = 0;
            for (int b = 0; b < B; b++) {
                const int left = new_tokens - count[b]; /* a pass emits up to n_draft + 1 tokens */
                n_draft[b] = -1;
                if (left <= 0) continue;
                const int k = speculate < left - 1 ? speculate : left - 1;
                d0[b] = nd;
                if (!spec_tree)
                    n_draft[b] = gpt2_ngram_draft(gen + (size_t)b * total, prompt_len + count[b], 3, 1, k, drafts + nd);
                else /* a path of depth d emits d + 1 tokens: no deeper than left - 1 */
                    n_draft[b] = k < 1 ? 0
                                       : gpt2_ngram_draft_tree(gen + (size_t)b * total, prompt_len + count[b], 3, 1, k,
                                                               tree_depth < k ? tree_depth : k, tree_branches,
                                                               drafts + nd, parents + nd);
                nd += n_draft[b];
                live++;
            }
            if (!live) break;
            if (spec_tree && spec_sampled
                    ? gpt2_decode_verify_tree_sampled(&model, drafts, parents, n_draft, n_acc, out, nodes, NULL)
                : spec_tree    ? gpt2_decode_verify_tree(&model, drafts, parents, n_draft, n_acc, out, nodes)
                : spec_sampled ? gpt2_decode_verify_sampled(&model, drafts, n_draft, n_acc, out, NULL)
                               : gpt2_decode_verify(&model, drafts, n_draft, n_acc, out, NULL))
                return 1;
            spec_passes++;
            spec_live += live;
            for (int b = 0; b < B; b++) {
                if (n_draft[b] < 0) continue;
                spec_accepted += n_acc[b];
                if (spec_tree && n_acc[b] > 0) {
                    /* is the node decoding continues from on the first-child chain from the root? */
                    const int last = nodes[b * HPA_VERIFY_MAX_ROWS + n_acc[b] - 1];
                    int cur = 0, on_first = 0;
                    for (int j = 0; j < n_draft[b] && !on_first; j++)
                        if (parents[d0[b] + j] == cur) { cur = j + 1; on_first = cur == last; }
                    spec_off_first += !on_first;
                }
                for (int i = 0; i <= n_acc[b]; i++) {
                    const int id = out[b * HPA_VERIFY_MAX_ROWS + i];
                    gen[(size_t)b * total + prompt_len + count[b]++] = id;
                    if (b == 0 && !quiet) print_token(&tk, id);
                }
                spec_tokens += n_acc[b] + 1;
            }
        }
        free(count); free(n_draft); free(n_acc); free(drafts); free(out); free(parents); free(nodes); free(d0);
    }
    int s0 = 0; /* the slot sequence 0 lives in; slot s holds sequence (s - s0 + B) % B */
    for (int t = 1; t < new_tokens && !speculate; t++) {
        if (!quiet) print_token(&tk, next[s0]);
        if (!quiet && logprobs) printf("[%.4f] ", lp[s0]);
        if (!quiet && top_lp) {
            print_alternatives(&tk, alt_ids + (size_t)s0 * top_lp, alt_lps + (size_t)s0 * top_lp, top_lp);
            printf("\n");
        }
        if (park_on && t == park_at) { /* t tokens are out: every sequence leaves the pool and comes back one slot on */
            GPT2Parked** parked = (GPT2Parked**)malloc(B * sizeof(GPT2Parked*));
            if (!parked) return 1;
            size_t bytes = 0;
            const double p0 = now_s();
            for (int b = 0; b < B; b++) {
                if (!(parked[b] = gpt2_decode_park(&model, b, 0))) return 1;
                bytes += gpt2_parked_bytes(parked[b]);
            }
            const double p1 = now_s();
            const int free_pages = gpt2_decode_free_pages(&model);
            for (int b = 0; b < B; b++)
                if (gpt2_decode_unpark(&model, parked[b], (b + 1) % B)) return 1;
            const double p2 = now_s();
            fprintf(stderr, "parked %d sequences of %d tokens (%.1f MB of K/V) in %.3f ms: %d of %d pages free; "
                            "unparked into slots (b + 1) %% %d in %.3f ms\n", B, gpt2_parked_tokens(parked[0]),
                    1e-6 * (double)bytes, 1e3 * (p1 - p0), free_pages, B * max_pages, B, 1e3 * (p2 - p1));
            if (free_pages != B * max_pages) { fprintf(stderr, "the pool is not empty after parking\n"); return 1; }
            for (int b = 0; b < B; b++) gpt2_parked_free(parked[b]);
            free(parked);
            s0 = 1 % B;
        }
        /* the previous ids stay on the device and feed this step */
        if (gpt2_decode_step(&model, NULL, next)) return 1;
        if (logprobs && gpt2_decode_logprobs(&model, lp)) return 1;
        if (top_lp && gpt2_decode_top_logprobs(&model, alt_ids, alt_lps)) return 1;
        for (int b = 0; b < B; b++) gen[(size_t)b * total + prompt_len + t] = next[(b + s0) % B];
    }
    if (!quiet && new_tokens > 0 && !speculate) print_token(&tk, next[s0]);
    if (!quiet && logprobs && new_tokens > 0) printf("[%.4f] ", lp[s0]);
    if (!quiet && top_lp && new_tokens > 0)
        print_alternatives(&tk, alt_ids + (size_t)s0 * top_lp, alt_lps + (size_t)s0 * top_lp, top_lp);
    double t2 = now_s();
    if (!quiet) printf("\n---\nFinished!\n");
    printf("prefill %d x %d tokens in %.3f ms; generated %d tokens x %d sequences (%s) in %.3f ms: "
           "%.1f tokens/s\n", B, prompt_len, 1e3 * (t1 - t0), new_tokens, B, greedy ? "greedy" : "sampled",
           1e3 * (t2 - t0), new_tokens > 1 ? (double)(new_tokens - 1) * B / (t2 - t1) : 0.0);
    if (speculate)
        printf("speculation: %ld passes, %ld tokens emitted, mean accepted %.2f drafts per sequence and pass\n",
               spec_passes, spec_tokens, spec_live ? (double)spec_accepted / spec_live : 0.0);
    if (spec_tree)
        printf("tree speculation: %ld of %ld (sequence, pass) pairs continued from a node off the first branch\n",
               spec_off_first, spec_live);
    if (ids_out) {
        FILE* f = fopen(ids_out, "wb");
        if (!f || fwrite(gen, sizeof(int), (size_t)B * total, f) != (size_t)B * total) return 1;
        fclose(f);
    }
    tokenizer_free(&tk);
    free(gen);
    free(prompt);
    free(next);
    free(lp);
    free(alt_ids);
    free(alt_lps);
    gpt2_free(&model);         /* does not free the manager (reference ownership) */
    destroy_block_manager(bm);
    return 0;
}
