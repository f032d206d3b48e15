'use strict';
/* The draw list from the JavaScript host, on a GPU (driven by tests/test_gpu_draw_list.py):
 *     node tests/js/draw_list_gpu.js job.json
 * job: { w, h, dir, feeds: [{file (one packed frame), want (the expected canvas, RGBA), width, height, format, matrix, rect | null, wb}] } —
 * expectations by the declared conversion + the oracle.
 *  1. ccv.DeviceBatch with mixed opts.sources: uploadSourceOf + drawList into a frame set; getWhitebalance of that set is the oracle's value
 *     on the expected canvases, and detectStep on it equals detectStep of a second batch that got the expected canvases by upload();
 *  2. drawListBound + the step functions at set = -1: the same;
 *  3. only drawListDevice is called, never a single-source draw; a rect outside its source is refused with HT_ERR_INVALID and names the
 *     entry; the batch is usable afterwards.
 * Prints "draw_list_gpu: ok" or the failed checks. */
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
const n = job.feeds.length, fb = job.w * job.h * 4;

let listDraws = 0, otherDraws = 0;
const realList = A.drawListDevice, realYuv = A.drawFramesYuvDevice, realRgba = A.drawFramesDevice;
check(typeof realList === 'function' && A.DRAW_RGBA === 16, 'addon exports');
A.drawListDevice = function () { listDraws++; return realList.apply(this, arguments); };
A.drawFramesYuvDevice = function () { otherDraws++; return realYuv.apply(this, arguments); };
A.drawFramesDevice = function () { otherDraws++; return realRgba.apply(this, arguments); };

const sources = job.feeds.map(function (f) { return { width: f.width, height: f.height, format: f.format, matrix: f.matrix, sets: 2 }; });
const rects = job.feeds.map(function (f) { return f.rect; });
const want = new Uint8Array(n * fb);
job.feeds.forEach(function (f, i) { want.set(new Uint8Array(fs.readFileSync(path.join(job.dir, f.want))), i * fb); });

/* the reference batch: the expected canvases, uploaded directly */
const ref = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: 1, sets: 1 });
ref.upload(want, 0);
const refWb = ref.whitebalance(0), refBest = ref.detectStep(0).best;
job.feeds.forEach(function (f, i) { check(refWb[i] === f.wb, 'the uploaded canvas ' + i + ' has the oracle\'s whitebalance'); });

const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: 1, sets: 2, sources: sources });
job.feeds.forEach(function (f, i) { b.uploadSourceOf(i, new Uint8Array(fs.readFileSync(path.join(job.dir, f.file))), 1); });
b.drawList(1, 1, rects);
check(same(b.whitebalance(1), refWb), 'whitebalance of the set drawList drew');
check(same(b.detectStep(1).best, refBest), 'detectStep on the set drawList drew');
b.drawListBound(1, rects);
check(same(b.whitebalance(-1), refWb), 'whitebalance after drawListBound');
check(same(b.detectStep(-1).best, refBest), 'detectStep(-1) after drawListBound');
check(listDraws === 2 && otherDraws === 0, 'the facade must call drawListDevice and no single-source draw (' + listDraws + ', ' + otherDraws + ')');
let threw = false;
try { b.drawList(1, 0, rects.map(function (r, i) { return i === 1 ? [0, 0, job.feeds[1].width + 1, 1] : r; })); } catch (e) { threw = /status -1/.test(e.message) && /entry 1:/.test(e.message); }
check(threw, 'a rect outside its source is refused with HT_ERR_INVALID, naming entry 1');
b.drawList(1, 0, rects);
check(same(b.whitebalance(0), refWb), 'usable after the refused draw');
b.destroy();
ref.destroy();

process.stdout.write(errors.length ? JSON.stringify({ ok: false, checks: checks, errors: errors }) + '\n' : 'draw_list_gpu: ok (' + checks + ' checks)\n', function () { headtrackr.exitNow(errors.length ? 1 : 0); });
