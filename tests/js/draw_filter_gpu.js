'use strict';
/* The prefiltered draw list from the JavaScript host, on a GPU (driven by tests/test_gpu_draw_filter.py):
 *     node tests/js/draw_filter_gpu.js job.json
 * job: { w, h, dir, prefilter, feeds: [{file (one packed frame), want (the expected FILTERED canvas, RGBA), plain (the unfiltered one), width,
 *        height, format, matrix, rect | null, factors: [Nx, Ny]}] } — expectations by the Python restatement.
 *  1. ccv.DeviceBatch with mixed opts.sources: drawList(sset, set, rects, {prefilter}) into a frame set — the set's bytes, downloaded, are the
 *     expected filtered canvases, byte for byte; ONE drawListFilteredDevice call, no other draw; drawFilterFactors gives the expected factors;
 *  2. drawListBound(sset, rects, {prefilter}) + the step functions at set = -1 equal a batch that got the expected canvases by upload();
 *  3. without opts the same batch draws the unfiltered canvases through drawListDevice, as before; a prefilter of 9 throws before the addon;
 *     a rect outside its source is refused with HT_ERR_INVALID and names the entry; the batch is usable afterwards.
 * Prints "draw_filter_gpu: ok" or the failed checks. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const A = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr_hip.node'));
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const errors = [];
let checks = 0;
function check(cond, msg) { checks++; if (!cond && errors.length < 20) errors.push(msg); return cond; }
function same(a, b) { if (a.length !== b.length) return false; for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false; return true; }
function firstDiff(a, b) { for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return i; return -1; }
const n = job.feeds.length, fb = job.w * job.h * 4;

let filteredDraws = 0, listDraws = 0, otherDraws = 0;
const realFiltered = A.drawListFilteredDevice, realList = A.drawListDevice, realYuv = A.drawFramesYuvDevice, realRgba = A.drawFramesDevice;
check(typeof realFiltered === 'function' && typeof A.drawFilterFactors === 'function', 'addon exports');
A.drawListFilteredDevice = function () { filteredDraws++; return realFiltered.apply(this, arguments); };
A.drawListDevice = function () { listDraws++; return realList.apply(this, arguments); };
A.drawFramesYuvDevice = function () { otherDraws++; return realYuv.apply(this, arguments); };
A.drawFramesDevice = function () { otherDraws++; return realRgba.apply(this, arguments); };
/* the batch's context 0 and its frame-set buffer: the first context and the first device buffer it creates */
const made = { ctxs: [], devs: [] };
const realCreate = A.createContext, realAlloc = A.deviceAlloc;
A.createContext = function () { const c = realCreate.apply(this, arguments); made.ctxs.push(c); return c; };
A.deviceAlloc = function () { const d = realAlloc.apply(this, arguments); made.devs.push(d); return d; };

const sources = job.feeds.map(function (f) { return { width: f.width, height: f.height, format: f.format, matrix: f.matrix, sets: 1 }; });
const rects = job.feeds.map(function (f) { return f.rect; });
const read = function (key) { const a = new Uint8Array(n * fb); job.feeds.forEach(function (f, i) { a.set(new Uint8Array(fs.readFileSync(path.join(job.dir, f[key]))), i * fb); }); return a; };
const want = read('want'), plain = read('plain');
check(!same(want, plain), 'the filtered and the unfiltered expectation differ');

const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: 1, sets: 2, sources: sources });
const ctx0 = made.ctxs[0], setDev = made.devs[0];
job.feeds.forEach(function (f, i) { b.uploadSourceOf(i, new Uint8Array(fs.readFileSync(path.join(job.dir, f.file)))); });
const download = function (set) { const o = new Uint8Array(n * fb); A.deviceDownload(ctx0, setDev, set * n * fb, o); return o; };

b.drawList(0, 1, rects, { prefilter: job.prefilter });
let got = download(1);
check(same(got, want), 'drawList with opts.prefilter: every byte of the restatement (first difference at ' + firstDiff(got, want) + ')');
check(filteredDraws === 1 && listDraws === 0 && otherDraws === 0, 'ONE drawListFilteredDevice call and no other draw (' + [filteredDraws, listDraws, otherDraws] + ')');
check(same(b.drawFilterFactors(rects, { prefilter: job.prefilter }), [].concat.apply([], job.feeds.map(function (f) { return f.factors; }))), 'drawFilterFactors');

const ref = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: 1, sets: 1 });
ref.upload(want, 0);
const refWb = ref.whitebalance(0), refBest = ref.detectStep(0).best;
b.drawListBound(0, rects, { prefilter: job.prefilter });
check(same(b.whitebalance(-1), refWb), 'whitebalance after the filtered drawListBound');
check(same(b.detectStep(-1).best, refBest), 'detectStep(-1) after the filtered drawListBound');
check(filteredDraws === 2 && listDraws === 0, 'drawListBound took the filtered call');

b.drawList(0, 0, rects);
got = download(0);
check(same(got, plain), 'drawList without opts: the unfiltered canvases, as before');
check(same(download(1), want), 'set 1 still holds the filtered canvases');
check(filteredDraws === 2 && listDraws === 1 && otherDraws === 0, 'without opts the facade takes drawListDevice');
let threw = false;
try { b.drawList(0, 0, rects, { prefilter: 9 }); } catch (e) { threw = /opts\.prefilter is an integer 1\.\.8/.test(e.message); }
check(threw && filteredDraws === 2, 'a prefilter of 9 throws before the addon is reached');
threw = false;
try { b.drawList(0, 0, rects.map(function (r, i) { return i === 1 ? [0, 0, job.feeds[1].width + 1, 1] : r; }), { prefilter: job.prefilter }); } catch (e) { threw = /status -1/.test(e.message) && /entry 1:/.test(e.message); }
check(threw, 'a rect outside its source is refused with HT_ERR_INVALID, naming entry 1');
check(same(download(0), plain), 'the refused call wrote nothing');
b.drawList(0, 0, rects, { prefilter: job.prefilter });
check(same(download(0), want), 'usable after the refused draw');
b.destroy();
ref.destroy();

process.stdout.write(errors.length ? JSON.stringify({ ok: false, checks: checks, errors: errors }) + '\n' : 'draw_filter_gpu: ok (' + checks + ' checks)\n', function () { headtrackr.exitNow(errors.length ? 1 : 0); });
